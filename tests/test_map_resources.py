"""Register budget of the map-upkeep kernels (ygz_slam_amd/csrc/map.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory (the median is found by
counting over recomputed distances: no sorted row, no per-lane array), both kernels keep the eight wavefronts per SIMD DESIGN.md section 14
states and use no LDS."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _usage

# kernel -> (minimum wavefronts per SIMD, maximum VGPRs, maximum LDS bytes per block)
BUDGET = {"k_map_median": (8, 64, 0), "k_map_covis": (8, 16, 0)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_map_kernels_do_not_spill():
    u = _usage("map")
    assert len([k for k in u if "k_map_" in k]) == len(BUDGET)
    problems = []
    for key, (occ, vgprs, lds) in BUDGET.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if (v["ScratchSize"] != 0 or v["Occupancy"] < occ or v["VGPRs"] > vgprs or v["LDS Size"] > lds or v["VGPRs Spill"] != 0
                or v["SGPRs Spill"] != 0):
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (budget %d), %d VGPRs (budget %d), %d B of LDS (budget %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["LDS Size"], lds))
    assert not problems, "\n".join(problems)
