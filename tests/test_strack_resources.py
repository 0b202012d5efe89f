"""Register and LDS figures of the stereo tracking kernel (ygz_slam_amd/csrc/strack.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, no AGPRs, and the
figures are the ones DESIGN.md section 26 states.  The file has no atomic, no wait for another workgroup and no environment switch; the entry
point opens, uploads and fetches its packed block once each."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 26
FIGURES = {"k_strack_search": (6, 80, 16640)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_strack_kernel_does_not_spill():
    u = _usage("strack")
    assert len([k for k in u if "k_strack" in k]) == len(FIGURES)
    problems = []
    for key, (occ, vgprs, lds) in FIGURES.items():
        hits = [(k, v) for k, v in u.items() if re.search(r"\d%s(?![a-z_])" % key, k)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if (v["ScratchSize"] != 0 or v["Occupancy"] != occ or v["VGPRs"] != vgprs or v["AGPRs"] != 0 or v["LDS Size"] != lds
                or v["VGPRs Spill"] != 0 or v["SGPRs Spill"] != 0):
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (recorded %d), %d VGPRs (recorded %d), %d AGPRs, %d B of LDS (recorded %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["AGPRs"], v["LDS Size"], lds))
    assert not problems, "\n".join(problems)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert re.search(r"\| `k_strack_search` \| 256 \| 80 \| 0 \| 16640 \| 6 \| 0 \|", design)


def test_kernel_file_keeps_the_constraints():
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "strack.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    kernel = code[code.index("__global__"):code.index("static void strack_resolve")]
    for word in ["getenv", "atomic", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while (true)", "fma", "sin(", "cos("]:
        assert word not in code, word
    assert "float" not in kernel                                         # FP64 on the device; the rotation histogram's floats are host code
    assert "#pragma clang fp contract(off)" in hip and "-ffp-contract=off" in open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define\s+ST_LANES\s+256\b", hip) and re.search(r"#define\s+ST_TILE\s+256\b", hip) and "__launch_bounds__(ST_LANES)" in hip
    tile, group = (int(re.search(r"#define\s+%s\s+(\d+)" % n, hip).group(1)) for n in ("ST_TILE", "ST_GROUP"))
    assert group == 8 and tile % group == 0                              # the sweep reads whole groups; entries past the end are marked
    # one packed block, one upload, one launch, one copy back (which waits)
    assert code.count("ygz_blob_open(ctx, SCR_STRACK") == 1 and code.count("ygz_blob_upload(ctx, blob") == 1 and code.count("ygz_blob_fetch(ctx, blob") == 1
    assert code.count("ygz_blob_open(") == 1 and code.count("ygz_blob_upload(") == 1 and code.count("ygz_blob_fetch(") == 1
    assert code.count("YGZ_LAUNCH(") == 1 and "hipStreamSynchronize" not in code and "hipMemcpy" not in code
    # level and window first, then the gate, the Hamming distance last, the ladder after it; a block without a live point skips the sweep
    body = kernel[kernel.index("for (int t0 = 0; t0 < cnt; t0 += ST_GROUP)"):]
    assert body.index("lv <= hi") < body.index("dx < rad") < body.index("while (in_window)") < body.index("er > rad") < body.index("__popc(") < body.index("min(key[m], k)")
    assert "if (j >= n_kp) s_k[threadIdx.x].level = (int32_t)ST_TAKEN;" in code
    assert "__syncthreads_or(search)" in code and "(int)(blockIdx.x * ST_LANES) >= n_pt" in code
    # the other kernels' files are not this pull request's business: the registration only appends
    internal = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "ygz_internal.h")).read()
    assert "KID_LFUSE_SEARCH, KID_STRACK_SEARCH, KID_COUNT" in internal and "SCR_LFUSE, SCR_STRACK," in internal
