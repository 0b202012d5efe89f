"""Register and LDS figures of the stereo kernels (ygz_slam_amd/csrc/stereo.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory in either kernel;
k_stereo_match needs 41 VGPRs and 368 bytes of LDS (the 121-byte left patch and the 11 x 21 right strip of its one wavefront), k_stereo_median
22 VGPRs and 1064 bytes (a 256-bin histogram, the seven counts, three words of the selection): eight wavefronts per SIMD for both, the figures
DESIGN.md section 19 states.  The file reads no environment variable, has no float atomic (its only atomics count in LDS integers), no
cooperative launch, no wait for another workgroup and no fused multiply-add."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 19
FIGURES = {"k_stereo_match": (8, 41, 368), "k_stereo_median": (8, 22, 1064)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_stereo_kernels_do_not_spill():
    u = _usage("stereo")
    assert len([k for k in u if "k_stereo" in k]) == len(FIGURES)
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
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "stereo.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ["getenv", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while", "fma", "float"]:
        assert word not in code, word
    # the only atomics: integer counters in LDS (the two histograms and the counts per status)
    atomics = re.findall(r"atomic\w*\([^;]*;", code)
    assert len(atomics) == 3 and all(re.match(r"atomicAdd\(&s_(hist|cnt)\[", a) for a in atomics), atomics
    assert re.search(r"__shared__ unsigned s_hist\[256\];", code) and re.search(r"__shared__ int s_cnt\[YGZ_STEREO_N_STATUS\];", code)
    assert "#pragma clang fp contract(off)" in hip and "-ffp-contract=off" in open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define\s+ST_W\s+5\b", hip) and re.search(r"#define\s+ST_L\s+5\b", hip)
    assert hip.count("__launch_bounds__(64)") == 1 and hip.count("__launch_bounds__(256)") == 1
    # one wavefront per left keypoint, all pairs in one launch; one workgroup per pair for the median
    assert re.search(r"k_stereo_match, dim3\(\(unsigned\)stride, \(unsigned\)n_pairs\), dim3\(64\)", hip)
    assert re.search(r"k_stereo_median, dim3\(\(unsigned\)n_pairs\), dim3\(256\)", hip)
    # one upload, one copy back, one wait: the two calls of the blob helper and no transfer of the function's own; the helper's upload is one copy,
    # its fetch one copy and the one wait
    run = hip[hip.index("static int stereo_run"):hip.index("// the checks of the array form")]
    assert (run.count("ygz_blob_upload(") == 1 and run.count("ygz_blob_fetch(") == 1 and "hipMemcpyAsync(" not in run
            and "hipStreamSynchronize(" not in run)
    ctx = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "ctx.hip")).read()
    upload = ctx[ctx.index("int ygz_blob_upload("):ctx.index("int ygz_blob_fetch(")]
    fetch = ctx[ctx.index("int ygz_blob_fetch("):ctx.index("// ---- packed transfers")]
    assert upload.count("hipMemcpyAsync(") == 1 and "hipStreamSynchronize(" not in upload
    assert fetch.count("hipMemcpyAsync(") == 1 and fetch.count("hipStreamSynchronize(") == 1
