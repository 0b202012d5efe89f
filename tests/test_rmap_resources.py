"""Register, LDS, scratch and occupancy figures of the resident map's kernels (ygz_slam_amd/csrc/rmap.hip) from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile, asserted as equalities against the table of DESIGN.md
section 36: nothing spills to scratch memory, no AGPRs.  The file defines no kernel of the stages it launches, has no atomic and no unbounded
loop, and the shared host body gained its third source without a launch of its own."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 36
FIGURES = {"k_rmap_filter": (8, 22, 16), "k_rmap_scatter": (8, 12, 0)}
CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernels_match_the_table_and_do_not_spill():
    u = _usage("rmap")
    kernels = [k for k in u if re.search(r"\dk_", k)]
    assert len(kernels) == len(FIGURES), kernels                         # the kernels it launches from other files are not compiled here
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    problems = []
    for key, (occ, vgprs, lds) in FIGURES.items():
        hits = [(k, v) for k, v in u.items() if re.search(r"\d%s(?![a-z_])" % key, k)]
        assert len(hits) == 1, (key, [k for k, _ in hits])
        k, v = hits[0]
        if (v["ScratchSize"] != 0 or v["Occupancy"] != occ or v["VGPRs"] != vgprs or v["AGPRs"] != 0 or v["LDS Size"] != lds
                or v["VGPRs Spill"] != 0 or v["SGPRs Spill"] != 0):
            problems.append("%s: scratch %d B per lane, %d wavefronts per SIMD (recorded %d), %d VGPRs (recorded %d), %d AGPRs, %d B of LDS (recorded %d)"
                            % (k, v["ScratchSize"], v["Occupancy"], occ, v["VGPRs"], vgprs, v["AGPRs"], v["LDS Size"], lds))
        assert re.search(r"\| `%s` \| 256 \| %d \| 0 \| %d \| %d \| 0 \|" % (key, vgprs, lds, occ), design), key
    assert not problems, "\n".join(problems)


def test_kernel_file_keeps_the_constraints():
    hip = open(os.path.join(CSRC, "rmap.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ("getenv", "environ", "atomic", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while", "for (;;)", "fma",
                 "hipMemset", "ygz_scratch(", "ygz_blob_open("):
        assert word not in code, word
    defined = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", code)
    assert sorted(defined) == ["k_rmap_filter", "k_rmap_scatter"]
    # the stages are launched through their own files' launchers
    for call in ("ygz_lms_launch(", "ygz_mpa_launch(", "ygz_slm_launch_index", "ygz_slm_run("):
        assert call in code, call
    assert code.count("YGZ_LAUNCH(") == 2 and code.count("__shared__") == 1 and "__shared__ int32_t s_w[RM_WAVES]" in code
    # the resident call: two uploads and two copies back in all, one of each in the shared body; the hook makes the others and never waits
    hook = code[code.index("int resident_hook"):code.index("template <class T> void copy_rows")]
    assert hook.count("hipMemcpyAsync(") == 2 and "hipMemcpyHostToDevice" in hook and "hipMemcpyDeviceToHost" in hook and "Synchronize" not in hook
    call = code[code.index("int ygz_hip_stereo_local_map_resident"):]
    assert "hipMemcpy" not in call and "Synchronize" not in call and "YGZ_LAUNCH" not in call and call.count("ygz_slm_run(") == 1
    assert call.index("if (!ctx || !map_ok(ctx, map)) return YGZ_E_INVALID;") < call.index("ygz_slm_run(")
    # the filter bounds itself by the selection's count and the stride; lanes past a list's length do nothing in the stages behind it
    flt = code[code.index("void k_rmap_filter"):code.index("struct RmapScatterDev")]
    assert "min(max(A.n_pt0[f], 0), A.max_pt)" in flt and "if (i < n0)" in flt and "at >= 0 && at < n0" in flt
    idx = open(os.path.join(CSRC, "slm_index.hip")).read()
    strack = open(os.path.join(CSRC, "strack.hip")).read()
    assert "if (i >= t.n_pt) return;" in idx and "if ((int)(blockIdx.x * ST_LANES) >= n_pt) return;" in strack and "const bool live = i < n_pt;" in strack
    # the shared body: a third source, no launch of its own
    slm = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "slm.hip")).read())
    assert "src.resident(ctx, src.user, R)" in slm and "src.is_resident()" in slm
    share = open(os.path.join(CSRC, "slm_share.h")).read()
    assert "struct SlmResidentDev" in share and "int (*resident)(" in share
    internal = open(os.path.join(CSRC, "ygz_internal.h")).read()
    ctx = open(os.path.join(CSRC, "ctx.hip")).read()
    ids = re.search(r"enum \{ KID_BGR2GRAY = 0,(.*?)KID_COUNT \}", internal, re.S).group(0)
    names = re.search(r"k_kernel_names\[KID_COUNT\] = \{(.*?)\};", ctx, re.S).group(1)
    kids, kernels = re.findall(r"KID_\w+", ids)[:-1], re.findall(r'"(k_\w+)"', names)
    assert len(kids) == len(kernels)
    for kid, kernel in (("KID_RMAP_FILTER", "k_rmap_filter"), ("KID_RMAP_SCATTER", "k_rmap_scatter")):
        assert kids.index(kid) == kernels.index(kernel), kid
    assert re.search(r"#define\s+YGZ_N_SCRATCH\s+48\b", internal) and "ygz_rmap_free_all(ctx);" in ctx
