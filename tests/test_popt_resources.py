"""Register and LDS figures of the stereo pose optimisation's kernel (ygz_slam_amd/csrc/popt.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: k_pose_opt uses no scratch memory and spills neither vector
nor scalar registers.  Recorded, and stated in DESIGN.md section 20: 202 VGPRs, no AGPRs, 1664 bytes of LDS (4 x 28 wavefront sums, the 28 totals
and the solver's state), 2 wavefronts per SIMD -- one workgroup of 256 lanes is one wavefront per SIMD, so two frames share a compute unit's
SIMDs.  The message of the test carries the figures of the build at hand.  The file reads no environment variable, has no floating-point atomic
(its only atomics count in LDS integers), no cooperative launch, no wait for another workgroup and no fused multiply-add."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_pose_opt_kernel_does_not_spill():
    u = _usage("popt")
    hits = [(k, v) for k, v in u.items() if re.search(r"\dk_pose_opt(?![a-z_])", k)]
    assert len(hits) == 1, sorted(u)
    k, v = hits[0]
    figures = "%s: scratch %d B per lane, %d VGPRs spilled, %d SGPRs spilled; %d VGPRs, %d AGPRs, %d B of LDS, %d wavefronts per SIMD" % (
        k, v["ScratchSize"], v["VGPRs Spill"], v["SGPRs Spill"], v["VGPRs"], v["AGPRs"], v["LDS Size"], v["Occupancy"])
    print(figures)
    assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, figures
    assert v["Occupancy"] >= 1 and v["LDS Size"] <= 65536, figures


def test_kernel_file_keeps_the_constraints():
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "popt.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    # posemath_dev.h holds the rotation, the retraction and the level weight of this file: the same words are kept out of it
    shared = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "posemath_dev.h")).read()
    assert '#include "posemath_dev.h"' in hip and "#pragma clang fp contract(off)" in shared
    for word in ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while", "fma", "float", "sin(", "cos(", "exp(", "pow("]:
        assert word not in code and word not in re.sub(r"//[^\n]*", "", shared), word
    # the only atomics: the integer counters of a pass and of a classification, in LDS
    atomics = re.findall(r"atomic\w*\([^;]*;", code)
    assert len(atomics) == 3 and all(re.match(r"atomicAdd\(&S\.c_(ok|rej|inl), ", a) for a in atomics), atomics
    assert re.search(r"int c_ok, c_rej, c_inl;", code) and re.search(r"__shared__ PoptState S;", code)
    assert "#pragma clang fp contract(off)" in hip and "-ffp-contract=off" in open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "Makefile")).read()
    assert hip.count("__launch_bounds__(PT_THREADS)") == 1 and re.search(r"#define\s+PT_THREADS\s+256\b", hip)
    # one workgroup per frame, all frames of the call in one launch; one upload, one copy back, one wait
    assert re.search(r"k_pose_opt, dim3\(\(unsigned\)n_frames\), dim3\(PT_THREADS\)", hip) and hip.count("YGZ_LAUNCH(") == 1
    call = hip[hip.index('extern "C" int ygz_hip_optimize_pose_stereo'):]
    assert call.count("ygz_kcopy(") == 2 and call.count("hipStreamSynchronize(") == 1
    # every check before the device is touched
    assert call.index("YgzDeviceGuard") > call.index("pyramid_levels") > call.index("if (!ctx) return YGZ_E_INVALID;")
    # the probe table names the kernel
    assert '"k_pose_opt"' in open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "ctx.hip")).read()
