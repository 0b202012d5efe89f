"""Register budget of the projection-guided search's kernel (ygz_slam_amd/csrc/proj.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory (the eight-entry
candidate list is a min / max ladder over constant indices), the kernel keeps the eight wavefronts per SIMD DESIGN.md section 12 states, and
its LDS tile (256 keypoints: descriptor, level, pixel) leaves room for four blocks per compute unit."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _usage

# kernel -> (minimum wavefronts per SIMD, maximum VGPRs, maximum LDS bytes per block)
BUDGET = {"k_proj_search": (8, 64, 16384)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_proj_kernels_do_not_spill():
    u = _usage("proj")
    assert len([k for k in u if "k_proj_" in k]) == len(BUDGET)
    problems = []
    for key, (occ, vgprs, lds) in BUDGET.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if v["ScratchSize"] != 0 or v["Occupancy"] < occ or v["VGPRs"] > vgprs or v["LDS Size"] > lds or v["VGPRs Spill"] != 0:
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (budget %d), %d VGPRs (budget %d), %d B of LDS (budget %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["LDS Size"], lds))
    assert not problems, "\n".join(problems)
