"""Register and LDS figures of the stereo odometry kernels (ygz_slam_amd/csrc/svo.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, no AGPRs, and the
figures are the ones DESIGN.md section 27 tables.  The file holds no copy of k_strack_search or k_pose_opt, opens, uploads and fetches its
packed block once each, and has no floating-point atomic, no wait for another workgroup, no cooperative launch and no unbounded loop."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 27
FIGURES = {"k_svo_gather": (8, 40, 0), "k_svo_resolve": (8, 34, 13500), "k_svo_scatter": (8, 8, 0)}
SVO = os.path.join(ROOT, "ygz_slam_amd", "csrc", "svo.hip")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_svo_kernels_do_not_spill():
    u = _usage("svo")
    kernels = [k for k in u if re.search(r"\dk_", k)]
    assert len(kernels) == len(FIGURES), kernels                         # the two reused kernels are not compiled here
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
    hip = open(SVO).read()
    code = re.sub(r"//[^\n]*", "", hip)
    words = ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while (true)", "while(true)", "for (;;)", "fma",
             "hipStreamSynchronize", "hipMemcpy", "atomicAdd_system", "atomicCAS", "atomicExch"]
    for word in words:
        assert word not in code, word
    assert "while" not in code                                           # every loop is a for over a count known at entry
    # what the three slot trackers share is in one header, held to the same list: no atomic, no LDS of its own, no unbounded loop
    dev = re.sub(r"//[^\n]*", "", open(os.path.join(os.path.dirname(SVO), "slot_pose_dev.h")).read())
    for word in words + ["while", "atomic", "__shared__"]:
        assert word not in dev, word
    assert '#include "slot_pose_dev.h"' in hip
    # the two reused kernels are declared in the shared headers and defined in their own files: no copy here, and no kernel named after them
    assert '#include "strack_dev.h"' in hip and '#include "popt_dev.h"' in hip
    defined = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", code)
    assert sorted(defined) == ["k_svo_gather", "k_svo_resolve", "k_svo_scatter"] and not any("k_strack" in k or "k_pose_opt" in k for k in defined)
    for word in ("st_point", "pt_pass", "pt_solve6", "quat_to_R_d", "__popc("):
        assert word not in code, word
    assert code.count("k_strack_search,") == 1 and code.count("k_pose_opt,") == 1       # launched, once each in the text (the search inside the pass loop)
    # integer atomics on LDS counters only: every atomic is an atomicAdd of an int into a __shared__ int array
    atomics = re.findall(r"atomic\w*\([^;]*;", code)
    assert len(atomics) == 6 and all(re.match(r"atomicAdd\(&s_(hist|cnt)\[[^\]]+\], (1|c_\w+)\);", a) for a in atomics), atomics
    assert re.search(r"__shared__ int s_hist\[30\], s_ind\[3\], s_cnt\[SV_N_COUNTERS\]", code)
    assert "#pragma clang fp contract(off)" in hip
    assert re.search(r"#define\s+SV_LANES\s+256\b", hip) and hip.count("__launch_bounds__(SV_LANES)") == 3
    # one packed block: one open, one upload, one copy back (which waits)
    assert code.count("ygz_blob_open(ctx, SCR_SVO") == 1 and code.count("ygz_blob_open(") == 1
    assert code.count("ygz_blob_upload(") == 1 and code.count("ygz_blob_fetch(") == 1
    call = code[code.index("int ygz_hip_stereo_odometry_slots"):]
    # every check before the device is touched, the context last; no host decision between the upload and the copy back
    assert call.index("if (!ctx) return YGZ_E_INVALID;") < call.index("pyr_valid") < call.index("YgzDeviceGuard") < call.index("ygz_blob_upload(")
    between = call[call.index("ygz_blob_upload("):call.index("ygz_blob_fetch(")]
    assert "hipMemcpy" not in between and "Synchronize" not in between and between.count("YGZ_LAUNCH(") == 5
    assert "for (int pass = 0; pass < 2; ++pass)" in between             # both passes are launched whatever the first one found
    # the keys' indices are checked against n_kp before they address anything
    resolve = code[code.index("void k_svo_resolve"):code.index("void k_svo_scatter")]
    assert "j_ < (uint32_t)n_kp" in resolve and resolve.count("m >= n_kp") == 2 and "m < n_kp" in resolve
