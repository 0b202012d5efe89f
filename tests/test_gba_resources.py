"""Register budget of the global bundle adjustment's kernels (ygz_slam_amd/csrc/gba.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory (the 3x3 and 6x6 blocks,
the Cholesky factor and the accumulators have constant indices only), and every kernel keeps the occupancy DESIGN.md section 15 states.  The
two kernels that tree-sum 27 quantities per pose hold 27 x 256 doubles of LDS (54 KiB): two workgroups per CU."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> minimum wavefronts per SIMD
BUDGET = {"k_gba_linearize": 4, "k_gba_point_system": 8, "k_gba_pose_system": 2, "k_gba_begin": 8, "k_gba_point_trial": 8, "k_gba_pose_trial": 2,
          "k_gba_cg_begin": 4, "k_gba_cg_point": 4, "k_gba_cg_pose": 6, "k_gba_cg_step": 4, "k_gba_point_update": 4, "k_gba_pose_update": 8,
          "k_gba_cost": 8, "k_gba_decide": 8, "k_gba_accept": 8}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_gba_kernels_do_not_spill():
    u = _usage("gba")
    assert len([k for k in u if "k_gba_" in k]) == len(BUDGET)
    problems = []
    for key, occ in BUDGET.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if v["ScratchSize"] != 0 or v["Occupancy"] < occ:
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (budget %d), %d VGPRs" % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"]))
        assert v.get("LDS Size", 0) <= 27 * 256 * 8 + 27 * 8                   # the largest reduction buffer, below the 64 KiB of a static allocation
    assert not problems, "\n".join(problems)


def test_summation_constants_are_shared_with_the_restatement():
    """the fixed summation order hangs on two numbers: the kernels' GBA_LANES and GBA_CHUNK are the restatement's GB_LANES and GB_CHUNK; the
    automatic CG cap's bound likewise.  No kernel of the file waits for another workgroup, and the file reads no environment variable"""
    import gba_ref as gb
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "gba.hip")).read()
    ref = open(os.path.join(ROOT, "tests", "gba_ref.c")).read()
    for dev, host, value in [("GBA_LANES", "GB_LANES", 256), ("GBA_CHUNK", "GB_CHUNK", 1024), ("GBA_CG_CAP", "GB_CG_CAP", 1024)]:
        assert int(re.search(r"#define\s+%s\s+(\d+)" % dev, hip).group(1)) == int(re.search(r"#define\s+%s\s+(\d+)" % host, ref).group(1)) == value
    assert (gb.LANES, gb.CHUNK, gb.CG_CAP) == (256, 1024, 1024)
    assert hip.count("__launch_bounds__(GBA_LANES)") == len(BUDGET)
    # gba_phases.h takes the rotation, the retraction and the Cholesky loops from posemath_dev.h: the same words are kept out of it
    shared = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "posemath_dev.h")).read()
    for text in (hip, shared):
        code = re.sub(r"//[^\n]*", "", text)
        for word in ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "atomicAdd", "__threadfence", "while ("]:
            assert word not in code, word
