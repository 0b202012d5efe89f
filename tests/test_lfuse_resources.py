"""Register and LDS figures of the local-map fusion kernel (ygz_slam_amd/csrc/lfuse.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, and the figures are the
ones DESIGN.md section 25 states.  The file has no atomic, no wait for another workgroup and no environment switch."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 25
FIGURES = {"k_lfuse_search": (6, 76, 16640)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_lfuse_kernel_does_not_spill():
    u = _usage("lfuse")
    assert len([k for k in u if "k_lfuse" in k]) == len(FIGURES)
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
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"\| `k_lfuse_search` \| 256 \| 76 \| 0 \| 16640 \| 6 \| 0 \|", design)


def LF_TILE_IS_WHOLE_GROUPS(hip):
    """the sweep reads whole groups: the tile must hold a whole number of them, and entries past the end are marked"""
    tile, group = (int(re.search(r"#define\s+%s\s+(\d+)" % n, hip).group(1)) for n in ("LF_TILE", "LF_GROUP"))
    return tile % group == 0


def test_kernel_file_keeps_the_constraints():
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "lfuse.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ["getenv", "atomic", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while (true)", "fma", "float", "sin(", "cos("]:
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in hip and "-ffp-contract=off" in open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define\s+LF_LANES\s+256\b", hip) and re.search(r"#define\s+LF_TILE\s+256\b", hip) and "__launch_bounds__(LF_LANES)" in hip
    # one packed block, one upload, one launch, one copy back (which waits)
    assert code.count("ygz_blob_open(ctx, SCR_LFUSE") == 1 and code.count("ygz_blob_upload(ctx, blob") == 1 and code.count("ygz_blob_fetch(ctx, blob") == 1
    assert code.count("YGZ_LAUNCH(") == 1 and "hipStreamSynchronize" not in code and "hipMemcpy" not in code
    # level and window first, then the gate, the Hamming distance last; a block without a live point skips the sweep
    body = code[code.index("for (int t0 = 0; t0 < cnt; t0 += LF_GROUP)"):]
    assert body.index("lv <= pred") < body.index("dx < rad") < body.index("while (in_window)") < body.index("chi2_stereo") < body.index("__popc(")
    assert "if (j >= n_kp) s_k[threadIdx.x].level = (int32_t)LF_TAKEN;" in code and LF_TILE_IS_WHOLE_GROUPS(hip)
    assert "__syncthreads_or(pred >= 0)" in code and "(int)(blockIdx.x * LF_LANES) >= n_pt" in code
