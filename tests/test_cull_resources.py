"""Register and LDS figures of the keyframe-culling kernels (ygz_slam_amd/csrc/cull.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory in either kernel;
k_cull_counts holds its 2 x 4096 counters in exactly 32 KiB of LDS (five workgroups of four wavefronts per CU: the five wavefronts per SIMD
DESIGN.md section 17 states) in 22 VGPRs, k_cull_walk its removed flags and three sum slots in 4120 bytes in 18 VGPRs (one workgroup of
sixteen wavefronts: four per SIMD are resident, eight would fit).  The file has no floating-point atomic, no wait for another workgroup and no
environment switch."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 17
FIGURES = {"k_cull_counts": (5, 22, 2 * 4096 * 4), "k_cull_walk": (8, 18, 4096 + 3 * 2 * 4)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_cull_kernels_do_not_spill():
    u = _usage("cull")
    assert len([k for k in u if "k_cull_" in k]) == len(FIGURES)
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
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "cull.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert int(re.search(r"#define\s+YGZ_CULL_MAX_KEYFRAMES\s+(\d+)", hdr).group(1)) == 4096
    assert "__shared__ int32_t s_cnt[2 * YGZ_CULL_MAX_KEYFRAMES]" in hip and "__shared__ uint8_t s_removed[YGZ_CULL_MAX_KEYFRAMES]" in hip
    assert hip.count("__launch_bounds__(CULL_LANES)") == 1 and hip.count("__launch_bounds__(CULL_WALK_LANES)") == 1
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "atomicCAS", "float", "while"]:
        assert word not in code, word
    # every atomic adds an integer: three in LDS, one per non-zero counter in global memory
    atomics = re.findall(r"atomic\w+\s*\(([^;]*);", code)
    assert len(atomics) == 5 and len(re.findall(r"\batomicAdd\b", code)) == 5 and len(re.findall(r"\batomic\w+", code)) == 5
    assert "double ratio" in code and code.count("(double)") == 2          # the one comparison
    # the walk is one workgroup: nothing to wait for
    assert re.search(r"k_cull_walk, dim3\(1\), dim3\(CULL_WALK_LANES\)", hip)
