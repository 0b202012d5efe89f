"""Register budgets of the Initializer's kernels (ygz_slam_amd/csrc/init.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, and each keeps the
occupancy DESIGN.md section 9 states (k_init_models is bounded by its 57.6 KB of LDS per 32-lane block, the single-lane k_init_decompose by
its registers: neither matters at 13 blocks and one block)."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _usage

# kernel -> minimum wavefronts per SIMD
BUDGET = {"k_init_normalize": 8, "k_init_models": 1, "k_init_score": 8, "k_init_sum": 8, "k_init_select": 8, "k_init_decompose": 2,
          "k_init_checkrt": 4, "k_init_parallax": 8, "k_init_accept": 8}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_init_kernels_do_not_spill():
    u = _usage("init")
    problems = []
    for key, occ in BUDGET.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if v["ScratchSize"] != 0 or v["Occupancy"] < occ:
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (budget %d), %d VGPRs" % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"]))
    assert not problems, "\n".join(problems)
