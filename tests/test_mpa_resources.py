"""Register, LDS, scratch and occupancy figures of the map-point attribute kernel (ygz_slam_amd/csrc/mpa.hip) and of the list gather of the
indexed local-map call (ygz_slam_amd/csrc/slm_index.hip), from the compiler's own remarks (-Rpass-analysis=kernel-resource-usage) for the flags
of ygz_slam_amd/csrc/Makefile, asserted as equalities against the table of DESIGN.md section 35: nothing spills to scratch memory, no AGPRs,
no LDS.  The files keep their constraints: FP64 uncontracted, no atomic, no environment switch, one upload, one copy back."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# file -> kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 35
FIGURES = {"mpa": {"k_mpa_attr": (8, 60, 0)}, "slm_index": {"k_slm_index": (8, 12, 0)}}
CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("name", sorted(FIGURES))
def test_kernels_match_the_table_and_do_not_spill(name):
    u = _usage(name)
    kernels = [k for k in u if re.search(r"\dk_", k)]
    assert len(kernels) == len(FIGURES[name]), kernels                   # no other kernel is compiled in the file
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    problems = []
    for key, (occ, vgprs, lds) in FIGURES[name].items():
        hits = [(k, v) for k, v in u.items() if re.search(r"\d%s(?![a-z_])" % key, k)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if (v["ScratchSize"] != 0 or v["Occupancy"] != occ or v["VGPRs"] != vgprs or v["AGPRs"] != 0 or v["LDS Size"] != lds
                or v["VGPRs Spill"] != 0 or v["SGPRs Spill"] != 0):
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (recorded %d), %d VGPRs (recorded %d), %d AGPRs, %d B of LDS (recorded %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["AGPRs"], v["LDS Size"], lds))
        assert re.search(r"\| `%s` \| 256 \| %d \| 0 \| %d \| %d \| 0 \|" % (key, vgprs, lds, occ), design), key
    assert not problems, "\n".join(problems)


def test_kernel_files_keep_the_constraints():
    mpa = open(os.path.join(CSRC, "mpa.hip")).read()
    idx = open(os.path.join(CSRC, "slm_index.hip")).read()
    slm = open(os.path.join(CSRC, "slm.hip")).read()
    share = open(os.path.join(CSRC, "slm_share.h")).read()
    for text in (mpa, idx, share):
        code = re.sub(r"//[^\n]*", "", text)
        for word in ("getenv", "environ", "atomic", "__shared__", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while", "fma",
                     "hipMemcpy", "hipMemset", "hipStreamSynchronize"):
            assert word not in code, word
    code = re.sub(r"//[^\n]*", "", mpa)
    assert "#pragma clang fp contract(off)" in mpa and re.search(r"#define\s+SCR_MPA\s+47\b", mpa) and "ygz_blob_open(ctx, SCR_MPA" in mpa
    assert code.count("ygz_blob_upload(") == 1 and code.count("ygz_blob_fetch(") == 1 and code.count("YGZ_LAUNCH(") == 1
    # the order of the additions: the squares left to right, the sum in row order
    assert re.search(r"double q = r0 \* r0;\s*q = q \+ r1 \* r1;\s*q = q \+ r2 \* r2;\s*const double d = sqrt\(q\);", code)
    assert "s0 += r0 / d; s1 += r1 / d; s2 += r2 / d;" in code and "for (int e = a; e < b; ++e)" in code
    call = code[code.index("int ygz_hip_map_point_attributes"):]
    assert call.index("if (!ctx) return YGZ_E_INVALID;") < call.index("YgzDeviceGuard") < call.index("ygz_blob_open(") < call.index("ygz_blob_upload(")
    # the list gather copies and computes nothing; the host body of the two local-map entry points exists once, in slm.hip
    code = re.sub(r"//[^\n]*", "", idx)
    assert "sqrt" not in code and " / " not in code and "pragma" not in code
    assert code.count("YGZ_LAUNCH(") == 1 and "ygz_blob_" not in code and code.count("ygz_slm_run(") == 1 and '#include "slm_share.h"' in idx
    assert re.sub(r"//[^\n]*", "", slm).count("ygz_slm_run(") == 2 and "int ygz_slm_run(" in share and '#include "slm_share.h"' in slm
    internal = open(os.path.join(CSRC, "ygz_internal.h")).read()
    ctx = open(os.path.join(CSRC, "ctx.hip")).read()
    ids = re.search(r"enum \{ KID_BGR2GRAY = 0,(.*?)KID_COUNT \}", internal, re.S).group(0)
    names = re.search(r"k_kernel_names\[KID_COUNT\] = \{(.*?)\};", ctx, re.S).group(1)
    kids, kernels = re.findall(r"KID_\w+", ids)[:-1], re.findall(r'"(k_\w+)"', names)
    assert len(kids) == len(kernels)
    for kid, kernel in (("KID_MPA_ATTR", "k_mpa_attr"), ("KID_SLM_INDEX", "k_slm_index")):
        assert kids.index(kid) == kernels.index(kernel), kid
