"""Register and LDS figures of the rectification kernels (ygz_slam_amd/csrc/rectify.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory in any of the three;
the figures are the ones DESIGN.md section 23 states.  The file has no atomic, no wait for another workgroup and no environment switch, reads
the map's FP64 uncontracted, and takes the remap itself -- the map formula, the box, the tile's body -- from csrc/remap_dev.h, which it shares with
undistort.hip; tests/test_undistort_resources.py pins that the body exists once."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage
from test_undistort_resources import CSRC, read_code

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 23
FIGURES = {"k_rect_map": (8, 20, 0), "k_rect_boxes": (8, 24, 64), "k_rectify": (7, 67, 16384)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_rectify_kernels_do_not_spill():
    u = _usage("rectify")
    assert len([k for k in u if "k_rect" in k]) == len(FIGURES) and not [k for k in u if "k_undist" in k]
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
    hip, code = read_code("rectify.hip")
    hdr, hdr_code = read_code("remap_dev.h")
    for word in ["getenv", "atomic", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while", "fma", "float"]:
        assert word not in code and word not in hdr_code, word
    assert "k_undist" not in code
    assert "#pragma clang fp contract(off)" in hip and "#pragma clang fp contract(off)" in hdr
    assert "-ffp-contract=off" in open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"#define\s+RM_TW\s+64\b", hdr) and re.search(r"#define\s+RM_TH\s+32\b", hdr) and re.search(r"#define\s+RM_LDS\s+16384\b", hdr)
    assert not re.search(r"#define\s+(UD|RC|RM)_", hip)
    img = open(os.path.join(CSRC, "image.hip")).read()
    assert re.search(r"#define\s+PD_TW\s+64\b", img) and re.search(r"#define\s+PD_TH\s+32\b", img)          # the tile of k_pyr_down
    assert hip.count("__launch_bounds__(256)") == 3 and "__shared__ __attribute__((aligned(16))) uint8_t tile[RM_LDS]" in hip
    # one device function makes the map's integers: defined once in the header, called once here
    assert code.count("remap_q(") == 1 and hdr_code.count("remap_q(") == 1 and "rint(" not in code and hdr_code.count("rint(") == 2
    # every tap is tested against the picture before it is read, and a box read from the table cannot index past the tile
    assert "(unsigned)x >= (unsigned)w || (unsigned)y >= (unsigned)h" in hdr_code and "& (RM_LDS - 1)]" in hdr_code
    # all slots of both cameras in one launch, the list through the packed-block helper
    assert re.search(r"dim3\(ygz_div_up\(w, RM_TW\), ygz_div_up\(h, RM_TH\), n_slots\)", hip)
    assert "ygz_blob_open(ctx, SCR_RECT" in code and "ygz_blob_upload(ctx, b" in code
