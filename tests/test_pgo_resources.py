"""Register budget of the pose-graph optimiser's kernel (ygz_slam_amd/csrc/pgo.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory (the 7x7 blocks, the
Cholesky factor and the gathers have constant indices only), and it keeps the occupancy DESIGN.md section 13 states.  k_pgo_optimize runs one
workgroup of 256 lanes per call, one wavefront per SIMD, so its occupancy of 1 is by design: the whole register file is its to use."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _usage

# kernel -> minimum wavefronts per SIMD
BUDGET = {"k_pgo_optimize": 1}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_pgo_kernel_does_not_spill():
    u = _usage("pgo")
    assert len([k for k in u if "k_pgo_" in k]) == len(BUDGET)
    problems = []
    for key, occ in BUDGET.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if v["ScratchSize"] != 0 or v["Occupancy"] < occ:
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (budget %d), %d VGPRs" % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"]))
    assert not problems, "\n".join(problems)
    # one workgroup of 256 lanes: the LDS it declares is the reduction buffer, far below a CU's
    assert hits[0][1].get("LDS Size", 0) <= 4096


def test_lane_count_is_shared_with_the_restatement():
    """the fixed summation order hangs on one number: the kernel's PGO_LANES is the restatement's PG_LANES, and the CG cap's bound likewise"""
    import re
    from conftest import ROOT
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "pgo.hip")).read()
    ref = open(os.path.join(ROOT, "tests", "pgo_ref.c")).read()
    lanes = int(re.search(r"#define\s+PGO_LANES\s+(\d+)", hip).group(1))
    assert lanes == int(re.search(r"#define\s+PG_LANES\s+(\d+)", ref).group(1)) == 256
    assert int(re.search(r"#define\s+PGO_CG_CAP\s+(\d+)", hip).group(1)) == int(re.search(r"#define\s+PG_CG_CAP\s+(\d+)", ref).group(1)) == 2048
    assert "__launch_bounds__(PGO_LANES)" in hip and "dim3(1), dim3(PGO_LANES)" in hip
