"""Register and LDS budget of the keyframe database's kernel (ygz_slam_amd/csrc/kfdb.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, the staged query
words take exactly YGZ_KFDB_MAX_WORDS x 4 bytes of LDS (32 KiB: five workgroups of four wavefronts per CU, the five wavefronts per SIMD
DESIGN.md section 16 states), at most 64 VGPRs.  The file has no floating-point atomic, no wait for another workgroup and no environment
switch."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (minimum wavefronts per SIMD, maximum VGPRs, LDS bytes per block)
BUDGET = {"k_kfdb_query": (5, 64, 8192 * 4)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_kfdb_kernel_does_not_spill():
    u = _usage("kfdb")
    assert len([k for k in u if "k_kfdb_" in k]) == len(BUDGET)
    problems = []
    for key, (occ, vgprs, lds) in BUDGET.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if (v["ScratchSize"] != 0 or v["Occupancy"] < occ or v["VGPRs"] > vgprs or v["LDS Size"] != lds or v["VGPRs Spill"] != 0
                or v["SGPRs Spill"] != 0):
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (budget %d), %d VGPRs (budget %d), %d B of LDS (stated %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["LDS Size"], lds))
    assert not problems, "\n".join(problems)


def test_kernel_file_keeps_the_constraints():
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "kfdb.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert int(re.search(r"#define\s+YGZ_KFDB_MAX_WORDS\s+(\d+)", hdr).group(1)) == 8192
    assert "__shared__ int32_t s_word[YGZ_KFDB_MAX_WORDS]" in hip and hip.count("__launch_bounds__(KFDB_LANES)") == len(BUDGET)
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "atomic", "__threadfence"]:
        assert word not in code, word
