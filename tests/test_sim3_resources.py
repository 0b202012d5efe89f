"""Register budgets of the loop detection's Sim3 kernels (ygz_slam_amd/csrc/sim3.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory (the Jacobi rotations,
the eigenvector pick, the 7x7 Cholesky and the 36 partial sums have constant indices only), and each keeps the occupancy DESIGN.md section 11
states.  k_sim3_refine runs one block per problem (at most 64 per call), so its single wavefront per SIMD is by design."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _usage

# kernel -> minimum wavefronts per SIMD
BUDGET = {"k_sim3_solve": 4, "k_sim3_score": 4, "k_sim3_select": 6, "k_sim3_refine": 1}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_sim3_kernels_do_not_spill():
    u = _usage("sim3")
    assert len([k for k in u if "k_sim3_" in k]) == len(BUDGET)
    problems = []
    for key, occ in BUDGET.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if v["ScratchSize"] != 0 or v["Occupancy"] < occ:
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (budget %d), %d VGPRs" % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"]))
    assert not problems, "\n".join(problems)
