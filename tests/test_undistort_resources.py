"""Register and LDS figures of the undistortion kernels (ygz_slam_amd/csrc/undistort.hip around the remap of csrc/remap_dev.h), from the compiler's
own remarks (-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory in either kernel;
k_undist_map needs 20 VGPRs and no LDS (eight wavefronts per SIMD); k_undistort stages a tile's source box in 16 KiB of LDS plus 64 bytes for
the four wavefronts' bounds (nine tiles per CU would fit, the 74 VGPRs admit six wavefronts per SIMD = six tiles per CU: the figures DESIGN.md
section 18 states).  The file and the header have no atomic, no wait for another workgroup and no environment switch, and read the map's FP64
uncontracted.  The remap's body -- the map formula, the box, the staging loop, the taps, the blend, the store -- exists once, in the header,
for this file and for rectify.hip."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 18
FIGURES = {"k_undist_map": (8, 20, 0), "k_undistort": (6, 74, 16384 + 64)}


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


CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")


def read_code(name):
    """a file of csrc: its text, and its text without // comments"""
    text = open(os.path.join(CSRC, name)).read()
    return text, re.sub(r"//[^\n]*", "", text)


def test_kernel_file_keeps_the_constraints():
    hip, code = read_code("undistort.hip")
    hdr, hdr_code = read_code("remap_dev.h")
    for word in ["getenv", "atomic", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while", "fma", "float"]:
        assert word not in code and word not in hdr_code, word
    assert "#pragma clang fp contract(off)" in hip and "#pragma clang fp contract(off)" in hdr
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"#define\s+RM_TW\s+64\b", hdr) and re.search(r"#define\s+RM_TH\s+32\b", hdr) and re.search(r"#define\s+RM_LDS\s+16384\b", hdr)
    assert not re.search(r"#define\s+(UD|RC|RM)_", hip)
    img = open(os.path.join(CSRC, "image.hip")).read()
    assert re.search(r"#define\s+PD_TW\s+64\b", img) and re.search(r"#define\s+PD_TH\s+32\b", img)          # the tile of k_pyr_down
    assert hip.count("__launch_bounds__(256)") == 2 and "__shared__ __attribute__((aligned(16))) uint8_t tile[RM_LDS]" in hip
    # one device function makes the map's integers, whoever asks: defined once in the header, called once here
    assert code.count("remap_q(") == 1 and hdr_code.count("remap_q(") == 1 and "rint(" not in code and hdr_code.count("rint(") == 2
    # every tap is tested against the picture before it is read, and a staged one cannot index past the tile
    assert "(unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h" in hdr_code and "& (RM_LDS - 1)]" in hdr_code
    # all slots in one launch
    assert re.search(r"dim3\(ygz_div_up\(w, RM_TW\), ygz_div_up\(h, RM_TH\), n_slots\)", hip)
    # every object depends on every header of csrc/, remap_dev.h (read above) among them
    assert "$(wildcard *.h)" in re.search(r"build/%\.o:[^\n]*", open(os.path.join(CSRC, "Makefile")).read()).group(0)


def test_the_remap_body_exists_once():
    """the blend and the gray weights occur once over the three files, in the header"""
    texts = {name: read_code(name)[1] for name in ("undistort.hip", "rectify.hip", "remap_dev.h")}
    for mark in ("+ 512) >> 10", "1868u"):
        assert {name: t.count(mark) for name, t in texts.items()} == {"undistort.hip": 0, "rectify.hip": 0, "remap_dev.h": 1}, mark
