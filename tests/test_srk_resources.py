"""Register and LDS figures of the stereo reference-keyframe kernels (ygz_slam_amd/csrc/srk.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, no AGPRs, and the
figures are the ones DESIGN.md section 29 tables.  The file holds no copy of k_bow_transform, k_bow_match or k_pose_opt, opens, uploads and
fetches its packed block once each, and has integer atomics only, no wait for another workgroup, no cooperative launch and no unbounded
loop."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 29
FIGURES = {"k_srk_gather": (8, 24, 0), "k_srk_resolve": (8, 34, 188), "k_srk_scatter": (8, 8, 0)}
CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")
SRK = os.path.join(CSRC, "srk.hip")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_srk_kernels_do_not_spill():
    u = _usage("srk")
    kernels = [k for k in u if re.search(r"\dk_", k)]
    assert len(kernels) == len(FIGURES), kernels                         # the three reused kernels are not compiled here
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
    hip = open(SRK).read()
    code = re.sub(r"//[^\n]*", "", hip)
    words = ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "for (;;)", "fma", "hipStreamSynchronize",
             "hipMemcpy", "atomicAdd_system", "atomicCAS", "atomicExch", "atomicOr", "atomicMax"]
    for word in words:
        assert word not in code, word
    assert "while" not in code                                           # every loop is a for over a count known at entry
    # what the three slot trackers share is in one header, held to the same list: no atomic, no LDS of its own, no unbounded loop
    dev = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "slot_pose_dev.h")).read())
    for word in words + ["while", "atomic", "__shared__"]:
        assert word not in dev, word
    assert '#include "slot_pose_dev.h"' in hip
    # the three reused kernels are declared in the shared headers and defined in their own files: no copy here, and no kernel named after them
    assert '#include "bow_dev.h"' in hip and '#include "popt_dev.h"' in hip and '#include "ur_dev.h"' in hip
    defined = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", code)
    assert sorted(defined) == ["k_srk_gather", "k_srk_resolve", "k_srk_scatter"]
    for word in ("bow_dist", "pt_pass", "pt_solve6", "quat_to_R_d", "__popc(", "child_off["):
        assert word not in code, word
    assert code.count("k_bow_transform,") == 1 and code.count("k_bow_match<0>,") == 1 and code.count("k_pose_opt,") == 1     # launched, once each
    # bow.hip keeps the definitions and gives the instantiation the header declares; the header defines no kernel
    bow = open(os.path.join(CSRC, "bow.hip")).read()
    dev = open(os.path.join(CSRC, "bow_dev.h")).read()
    assert '#include "bow_dev.h"' in bow and "struct BowPair" not in bow and "struct VocDev" not in bow and "struct ygz_hip_ctx::Vocab" not in bow
    assert "struct BowPair" in dev and "struct VocDev" in dev and "struct ygz_hip_ctx::Vocab" in dev
    assert re.search(r"extern template __global__ void k_bow_match<0>\(", dev) and re.search(r"\ntemplate __global__ void k_bow_match<0>\(", bow)
    assert "{" not in re.sub(r"struct [^;]*?\{.*?\};", "", re.sub(r"//[^\n]*", "", dev), flags=re.S)
    # integer atomics only: one atomicMin on the frame's int32 holder row, atomicAdds of ints into __shared__ int arrays
    atomics = re.findall(r"atomic\w*\([^;]*;", code)
    assert len(atomics) == 7, atomics
    assert atomics.count("atomicMin(&holder[m], i);") == 1 and atomics.count("atomicAdd(&s_hist[bin], 1);") == 1
    assert sum(1 for a in atomics if re.match(r"atomicAdd\(&s_cnt\[SR_N_\w+\], c_\w+\);", a)) == 5
    assert re.search(r"__shared__ int s_hist\[30\], s_ind\[3\], s_cnt\[SR_N_COUNTERS\], s_wave\[SR_LANES / 64\]", code)
    assert re.search(r"int32_t \*m12 = A.match12 \+ kb, \*holder = A.holder \+ kb;", code) and "double *holder" not in code
    assert "#pragma clang fp contract(off)" in hip
    assert re.search(r"#define\s+SR_LANES\s+256\b", hip) and hip.count("__launch_bounds__(SR_LANES)") == 3
    # one packed block: one open, one upload, one copy back (which waits)
    assert code.count("ygz_blob_open(ctx, SCR_SRK") == 1 and code.count("ygz_blob_open(") == 1
    assert code.count("ygz_blob_upload(") == 1 and code.count("ygz_blob_fetch(") == 1
    call = code[code.index("int ygz_hip_stereo_ref_keyframe_slots"):]
    # every check before the device is touched, the context last; no host decision between the upload and the copy back
    assert (call.index("if (!ctx) return YGZ_E_INVALID;") < call.index("if (!ctx->vocab) return YGZ_E_STATE;") < call.index("pyr_valid")
            < call.index("YgzDeviceGuard") < call.index("ygz_blob_upload("))
    between = call[call.index("ygz_blob_upload("):call.index("ygz_blob_fetch(")]
    assert "hipMemcpy" not in between and "Synchronize" not in between and between.count("YGZ_LAUNCH(") == 7
    launches = between[between.index("YGZ_LAUNCH("):between.rindex(";") + 1]      # up to the end of the last launch
    assert not re.search(r"\b(if|for|switch)\s*\(", launches) and "?" not in launches
    order = re.findall(r"YGZ_LAUNCH\(ctx, (KID_\w+),", launches)
    assert order == ["KID_SRK_GATHER", "KID_BOW_TRANSFORM", "KID_SRK_GATHER", "KID_BOW_MATCH", "KID_SRK_RESOLVE", "KID_POSE_OPT", "KID_SRK_SCATTER"]
    # every index read from kf_point or from a match is checked before it addresses anything
    resolve = code[code.index("void k_srk_resolve"):code.index("void k_srk_scatter")]
    assert "has && m >= 0 && m < n2" in resolve and "m < 0 || m >= n2 || holder[m] != i" in resolve and "r < 0 || r >= n2" in resolve
    assert "i >= 0 && i < n1 && A.outcome[kb + i] == 0" in resolve and "p >= 0 && p < n_pt" in resolve
    gather = code[code.index("void k_srk_gather"):code.index("enum { SR_N_UR")]
    assert "atomic" not in gather and "i < ygz_slot_count(A.n_kp, s, A.cells) && A.kf_point[" in gather
    # the right column of a resident keypoint is the shared header's
    assert "ygz_kp_right_column(" in code and "bf /" not in code
