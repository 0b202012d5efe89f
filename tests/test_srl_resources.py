"""Register and LDS figures of the stereo relocalisation kernels (ygz_slam_amd/csrc/srl.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, no AGPRs, and the
figures are the ones DESIGN.md section 32 tables.  The file holds no copy of k_bow_transform, k_bow_match, k_pose_opt or the three PnP
kernels, whose argument block and prototypes are in csrc/pnp_dev.h and whose definitions stay in pnp.hip; it opens, uploads and fetches its
packed block once each, and has integer atomics only, no wait for another workgroup, no cooperative launch and no unbounded loop."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 32
FIGURES = {"k_srl_gather": (8, 24, 0), "k_srl_resolve": (8, 34, 188), "k_srl_sets": (8, 12, 0), "k_srl_edges": (8, 31, 16),
           "k_srl_scatter": (8, 7, 0), "k_srl_pick": (8, 19, 0)}
CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")
SRL = os.path.join(CSRC, "srl.hip")
REUSED = ("k_bow_transform", "k_bow_match<0>", "k_pnp_solve", "k_pnp_score", "k_pnp_select", "k_pose_opt")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_srl_kernels_do_not_spill():
    u = _usage("srl")
    kernels = [k for k in u if re.search(r"\dk_", k)]
    assert len(kernels) == len(FIGURES), kernels                         # the six reused kernels are not compiled here
    problems = []
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
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
    hip = open(SRL).read()
    code = re.sub(r"//[^\n]*", "", hip)
    words = ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "for (;;)", "fma", "hipStreamSynchronize",
             "hipMemcpy", "atomicAdd_system", "atomicCAS", "atomicExch", "atomicOr", "atomicMax"]
    for word in words:
        assert word not in code, word
    assert "while" not in code                                           # every loop is a for over a count known at entry
    for inc in ("slot_pose_dev.h", "bow_dev.h", "popt_dev.h", "pnp_dev.h", "ur_dev.h", "cvrng_dev.h"):
        assert '#include "%s"' % inc in hip, inc
    # exactly the k_srl_ kernels are defined here, each with the 256-lane bound; the six reused ones are launched once each and defined nowhere
    # in this file, and nothing of their arithmetic stands here
    defined = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", code)
    assert sorted(defined) == sorted(FIGURES) and all(k.startswith("k_srl_") for k in defined)
    assert re.search(r"#define\s+SL_LANES\s+256\b", hip) and hip.count("__launch_bounds__(SL_LANES)") == len(FIGURES)
    for kern in REUSED:
        assert code.count(kern + ",") == 1, kern
    for word in ("bow_dist", "pt_pass", "pt_solve6", "quat_to_R_d", "__popc(", "child_off[", "pr_p3p", "pr_is_inlier", "pr_cubic_root", "root2real"):
        assert word not in code, word
    # pnp.hip keeps the definitions; the header declares the block and the three kernels and defines none
    pnp = open(os.path.join(CSRC, "pnp.hip")).read()
    dev = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "pnp_dev.h")).read())
    assert '#include "pnp_dev.h"' in pnp and "struct PnpDev" not in pnp and "struct PnpIn" not in pnp
    assert "struct PnpDev" in dev and "struct PnpIn" in dev and "const int32_t *end;" in dev and "const int32_t *skip;" in dev
    for k in ("k_pnp_solve", "k_pnp_score", "k_pnp_select"):
        assert re.search(r"__global__ void %s\(PnpDev D\);" % k, dev) and re.search(r"__global__ __launch_bounds__\(\w+\) void %s\(PnpDev D\)\s*\{" % k, pnp)
    assert dev.count("{") == 3                                           # the namespace and the two structs: no function body
    assert "D.end = nullptr; D.skip = nullptr;" in pnp                   # the host-array entry points use neither
    # integer atomics only: one atomicMin on the problem's int32 holder row, atomicAdds of ints into __shared__ int arrays
    atomics = re.findall(r"atomic\w*\([^;]*;", code)
    assert len(atomics) == 7, atomics
    assert atomics.count("atomicMin(&holder[m], i);") == 1 and atomics.count("atomicAdd(&s_hist[bin], 1);") == 1
    assert sum(1 for a in atomics if re.match(r"atomicAdd\(&s_cnt\[SL_N_\w+\], c_\w+\);", a)) == 5
    assert re.search(r"__shared__ int s_hist\[30\], s_ind\[3\], s_cnt\[SL_N_COUNTERS\], s_wave\[SL_LANES / 64\]", code)
    assert re.search(r"int32_t \*m12 = A.match12 \+ kb, \*holder = A.holder \+ kb;", code) and "double *holder" not in code
    assert "#pragma clang fp contract(off)" in hip
    # one packed block: one open, one upload, one copy back (which waits)
    assert code.count("ygz_blob_open(ctx, SCR_SRL") == 1 and code.count("ygz_blob_open(") == 1
    assert code.count("ygz_blob_upload(") == 1 and code.count("ygz_blob_fetch(") == 1
    call = code[code.index("int ygz_hip_stereo_relocalize_slots"):]
    # every check before the device is touched, the context last; no host decision between the upload and the copy back
    assert (call.index("if (!ctx) return YGZ_E_INVALID;") < call.index("if (!ctx->vocab) return YGZ_E_STATE;") < call.index("pyr_valid")
            < call.index("YgzDeviceGuard") < call.index("ygz_blob_upload("))
    between = call[call.index("ygz_blob_upload("):call.index("ygz_blob_fetch(")]
    assert "hipMemcpy" not in between and "Synchronize" not in between and between.count("YGZ_LAUNCH(") == 13
    launches = between[between.index("YGZ_LAUNCH("):between.rindex(";") + 1]      # up to the end of the last launch
    assert not re.search(r"\b(if|for|switch)\s*\(", launches) and "?" not in launches
    order = re.findall(r"YGZ_LAUNCH\(ctx, (KID_\w+),", launches)
    assert order == ["KID_SRL_GATHER", "KID_BOW_TRANSFORM", "KID_SRL_GATHER", "KID_BOW_MATCH", "KID_SRL_RESOLVE", "KID_SRL_SETS", "KID_PNP_SOLVE",
                     "KID_PNP_SCORE", "KID_PNP_SELECT", "KID_SRL_EDGES", "KID_POSE_OPT", "KID_SRL_SCATTER", "KID_SRL_PICK"]
    # every index read from kf_point, from a match or from an association is checked before it addresses anything
    resolve = code[code.index("void k_srl_resolve"):code.index("void k_srl_sets")]
    assert "has && m >= 0 && m < n2" in resolve and "m < 0 || m >= n2 || holder[m] != i" in resolve and "r < 0 || r >= n2" in resolve
    assert "i >= 0 && i < n1 && A.outcome[kb + i] == 0" in resolve and "p >= 0 && p < n_pt" in resolve
    edges = code[code.index("void k_srl_edges"):code.index("void k_srl_scatter")]
    assert "a >= 0 && a < n && a < cells && A.mask[kb + a] != 0" in edges
    sets = code[code.index("void k_srl_sets"):code.index("void k_srl_edges")]
    assert "!A.pnp_skip[q] && n >= 3" in sets and "if (it >= A.max_iter) return;" in sets
    # the right column of a resident keypoint is the shared header's
    assert "ygz_kp_right_column(" in code and "bf /" not in code
