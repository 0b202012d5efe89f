"""Register and LDS figures of the local-map selection kernels (ygz_slam_amd/csrc/lms.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory in any of the four;
k_lms_vote holds 4096 votes, the rank table, the list, a stage of eight covisible rows and six words in 33816 bytes of LDS (four workgroups of
four wavefronts per CU) in 16 VGPRs; k_lms_points and k_lms_prior hold the rank table (8 KiB) in 44 VGPRs, k_lms_place the rank table and
the scan of the counts (24 KiB) in 56.  The file has no floating point, no atomic on global memory, no wait for another workgroup and no
environment switch."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 34
FIGURES = {"k_lms_vote": (4, 16, 4096 * 4 + 2 * 4096 * 2 + 256 * 4 + 4 * 4 + 2 * 4), "k_lms_points": (8, 44, 4096 * 2 + 4 * 4),
           "k_lms_place": (6, 56, 4096 * 2 + 4096 * 4 + 4 * 4), "k_lms_prior": (8, 44, 4096 * 2)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_lms_kernels_do_not_spill():
    u = _usage("lms")
    assert len([k for k in u if "k_lms_" in k]) == len(FIGURES)
    problems = []
    for key, (occ, vgprs, lds) in FIGURES.items():
        hits = [(k, v) for k, v in u.items() if key + "E" in k or k.endswith(key)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if (v["ScratchSize"] != 0 or v["Occupancy"] != occ or v["VGPRs"] != vgprs or v["AGPRs"] != 0 or v["LDS Size"] != lds
                or v["VGPRs Spill"] != 0 or v["SGPRs Spill"] != 0):
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (recorded %d), %d VGPRs (recorded %d), %d B of LDS (recorded %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["LDS Size"], lds))
    assert not problems, "\n".join(problems)


def test_kernel_file_keeps_the_constraints():
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "lms.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert int(re.search(r"#define\s+YGZ_LMS_MAX_KEYFRAMES\s+(\d+)", hdr).group(1)) == 4096
    assert int(re.search(r"#define\s+YGZ_LMS_MAX_COV\s+(\d+)", hdr).group(1)) == 32
    assert "__shared__ int32_t s_votes[YGZ_LMS_MAX_KEYFRAMES]" in hip and hip.count("__shared__ uint16_t s_rank[YGZ_LMS_MAX_KEYFRAMES]") == 4
    assert hip.count("__launch_bounds__(LMS_LANES)") == 4 and "#pragma clang fp contract(off)" in hip
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ["getenv", "environ", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "atomicCAS", "float", "double", "while",
                 "hipMemset"]:
        assert word not in code, word
    # two atomics, both on integers in LDS: the vote and the reference keyframe's key
    assert re.findall(r"\batomic\w+\(&(\w+)", code) == ["s_votes", "s_best"] and len(re.findall(r"\batomic\w+", code)) == 2
    # one upload, four launches, one copy back
    assert code.count("ygz_blob_upload(") == 1 and code.count("ygz_blob_fetch(") == 1 and code.count("YGZ_LAUNCH(") == 4
    assert re.search(r"#define\s+SCR_LMS\s+46\b", hip) and "ygz_blob_open(ctx, SCR_LMS" in hip
