"""Register and LDS figures of the stereo local-map kernels (ygz_slam_amd/csrc/slm.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory, no AGPRs, and the
figures are the ones DESIGN.md section 28 tables.  The file holds no copy of k_strack_search or k_pose_opt, opens, uploads and fetches its
packed block once each, and has no floating-point atomic, no wait for another workgroup, no cooperative launch and no unbounded loop."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 28
FIGURES = {"k_slm_gather": (8, 41, 0), "k_slm_resolve": (8, 34, 16432), "k_slm_scatter": (8, 8, 0)}
CSRC = os.path.join(ROOT, "ygz_slam_amd", "csrc")
SLM = os.path.join(CSRC, "slm.hip")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_slm_kernels_do_not_spill():
    u = _usage("slm")
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
    hip = open(SLM).read()
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
    # the two reused kernels are declared in the shared headers and defined in their own files: no copy here, and no kernel named after them
    assert '#include "strack_dev.h"' in hip and '#include "popt_dev.h"' in hip and '#include "ur_dev.h"' in hip
    defined = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", code)
    assert sorted(defined) == ["k_slm_gather", "k_slm_resolve", "k_slm_scatter"] and not any("k_strack" in k or "k_pose_opt" in k for k in defined)
    for word in ("st_point", "pt_pass", "pt_solve6", "quat_to_R_d", "__popc("):
        assert word not in code, word
    assert code.count("k_strack_search,") == 1 and code.count("k_pose_opt,") == 1       # launched, once each
    # integer atomics on LDS counters only: every atomic is an atomicAdd of an int into a __shared__ int array
    atomics = re.findall(r"atomic\w*\([^;]*;", code)
    assert len(atomics) == 5 and all(re.match(r"atomicAdd\(&s_cnt\[SL_N_\w+\], c_\w+\);", a) for a in atomics), atomics
    assert re.search(r"__shared__ int s_oc\[SL_LANES\], s_cnt\[SL_N_COUNTERS\], s_wave\[SL_LANES / 64\]", code)
    assert "#pragma clang fp contract(off)" in hip
    assert re.search(r"#define\s+SL_LANES\s+256\b", hip) and hip.count("__launch_bounds__(SL_LANES)") == 3
    # one packed block: one open, one upload, one copy back (which waits)
    assert code.count("ygz_blob_open(ctx, SCR_SLM") == 1 and code.count("ygz_blob_open(") == 1
    assert code.count("ygz_blob_upload(") == 1 and code.count("ygz_blob_fetch(") == 1
    call = code[code.index("int ygz_hip_stereo_local_map_slots"):]
    # every check before the device is touched, the context last; no host decision between the upload and the copy back
    assert call.index("if (!ctx) return YGZ_E_INVALID;") < call.index("pyr_valid") < call.index("YgzDeviceGuard") < call.index("ygz_blob_upload(")
    between = call[call.index("ygz_blob_upload("):call.index("ygz_blob_fetch(")]
    assert "hipMemcpy" not in between and "Synchronize" not in between and between.count("YGZ_LAUNCH(") == 5
    launches = between[between.index("YGZ_LAUNCH("):between.rindex(";") + 1]      # up to the end of the last launch
    assert not re.search(r"\b(if|for|switch)\s*\(", launches) and "?" not in launches.replace("prior ? F : 0", "")
    # every index read from a key or from the prior is checked before it addresses anything
    resolve = code[code.index("void k_slm_resolve"):code.index("void k_slm_scatter")]
    assert resolve.count("j_ < (uint32_t)n_kp") == 1 and "< (uint32_t)n_kp) ? ((uint32_t)P.kp_level" in resolve and "if (pr >= n_pt) pr = -1;" in resolve
    assert "i >= 0 && i < n_pt" in resolve
    gather = code[code.index("void k_slm_gather"):code.index("void k_slm_resolve")]
    assert "pr >= 0 && pr < A.set_tab[A.fr_set[f]].n_pt" in gather and "atomic" not in gather
    # the right column of a resident keypoint is written once, in the header both gathering files include
    ur = open(os.path.join(CSRC, "ur_dev.h")).read()
    svo = open(os.path.join(CSRC, "svo.hip")).read()
    assert "return u - bf / z;" in ur and "has_mp != 0 && z > 0" in ur and '#include "ur_dev.h"' in svo
    assert "ygz_kp_right_column(" in svo and "ygz_kp_right_column(" in hip and "bf /" not in re.sub(r"//[^\n]*", "", svo) and "bf /" not in code
