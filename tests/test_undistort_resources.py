"""Register and LDS figures of the undistortion kernels (ygz_slam_amd/csrc/undistort.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory in either kernel;
k_undist_map needs 18 VGPRs and no LDS (eight wavefronts per SIMD); k_undistort stages a tile's source box in 16 KiB of LDS plus 64 bytes for
the four wavefronts' bounds (nine tiles per CU would fit, the 76 VGPRs admit six wavefronts per SIMD = six tiles per CU: the figures DESIGN.md
section 18 states).  The file has no atomic, no wait for another workgroup and no environment switch, and reads the map's FP64 uncontracted."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 18
FIGURES = {"k_undist_map": (8, 18, 0), "k_undistort": (6, 76, 16384 + 64)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_undistort_kernels_do_not_spill():
    u = _usage("undistort")
    assert len([k for k in u if "k_undist" in k]) == len(FIGURES)
    problems = []
    for key, (occ, vgprs, lds) in FIGURES.items():
        hits = [(k, v) for k, v in u.items() if re.search(r"\d%s(?![a-z_])" % key, k)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if (v["ScratchSize"] != 0 or v["Occupancy"] != occ or v["VGPRs"] != vgprs or v["AGPRs"] != 0 or v["LDS Size"] != lds
                or v["VGPRs Spill"] != 0 or v["SGPRs Spill"] != 0):
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (recorded %d), %d VGPRs (recorded %d), %d B of LDS (recorded %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["LDS Size"], lds))
    assert not problems, "\n".join(problems)


def test_kernel_file_keeps_the_constraints():
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "undistort.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ["getenv", "atomic", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while", "fma", "float"]:
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in hip and "-ffp-contract=off" in open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define\s+UD_TW\s+64\b", hip) and re.search(r"#define\s+UD_TH\s+32\b", hip) and re.search(r"#define\s+UD_LDS\s+16384\b", hip)
    img = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "image.hip")).read()
    assert re.search(r"#define\s+PD_TW\s+64\b", img) and re.search(r"#define\s+PD_TH\s+32\b", img)          # the tile of k_pyr_down
    assert hip.count("__launch_bounds__(256)") == 2 and "__shared__ __attribute__((aligned(16))) uint8_t tile[UD_LDS]" in hip
    # one device function makes the map's integers, whoever asks; every tap is tested against the picture before it is read
    assert code.count("undist_q(") >= 2 and "(unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h" in code
    # all slots in one launch
    assert re.search(r"dim3\(ygz_div_up\(w, UD_TW\), ygz_div_up\(h, UD_TH\), n_slots\)", hip)
