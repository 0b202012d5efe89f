"""Register and LDS figures of the map-point creation kernels (ygz_slam_amd/csrc/smap.hip), from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) for the flags of ygz_slam_amd/csrc/Makefile: nothing spills to scratch memory in either -- the 4 x 4
Jacobi of k_smap_pairs lives in registers -- and the figures are the ones DESIGN.md section 24 states.  The file has no atomic, no wait for
another workgroup and no environment switch, and restates the Jacobi instead of sharing init.hip's."""
import os
import re
import shutil

import pytest

from conftest import ROOT
from test_kernel_resources import HIPCC, _usage

# kernel -> (wavefronts per SIMD, VGPRs, LDS bytes per block): the figures the build reports, recorded in DESIGN.md section 24
FIGURES = {"k_smap_pairs": (3, 162, 132), "k_smap_keyframe": (7, 32, 2048)}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="hipcc not available")
def test_smap_kernels_do_not_spill():
    u = _usage("smap")
    assert len([k for k in u if "k_smap" in k]) == len(FIGURES)
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
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "smap.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    for word in ["getenv", "atomic", "hipLaunchCooperativeKernel", "cooperative_groups", "__threadfence", "while (true)", "fma", "float", "sin(", "cos(",
                 "atan", "ir_jacobi", '#include "init']:
        assert word not in code, word
    assert "#pragma clang fp contract(off)" in hip and "-ffp-contract=off" in open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "Makefile")).read()
    assert re.search(r"#define\s+SM_PAIR_THREADS\s+64\b", hip) and re.search(r"#define\s+SM_KF_THREADS\s+256\b", hip)
    assert "__launch_bounds__(SM_PAIR_THREADS)" in hip and "__launch_bounds__(SM_KF_THREADS)" in hip
    # the Jacobi is entered under the method's branch only, and its stop rule is the restatement's
    assert re.search(r"#define\s+SM_JACOBI_TOL\s+1e-15\b", hip) and re.search(r"#define\s+SM_JACOBI_SWEEPS\s+40\b", hip)
    ref = open(os.path.join(ROOT, "tests", "init_ref.c")).read()
    assert re.search(r"#define\s+IR_JACOBI_TOL\s+1e-15\b", ref) and re.search(r"#define\s+IR_JACOBI_SWEEPS\s+40\b", ref)
    assert code.count("sm_null_vector4(") == 2 and code.index("method = 1;") < code.rindex("sm_null_vector4(") < code.index("method = 2;")
    # each entry point: one packed block, one upload, one launch, one copy back (which waits)
    assert code.count("ygz_blob_open(ctx, SCR_SMAP") == 2 and code.count("ygz_blob_upload(ctx, b") == 2 and code.count("ygz_blob_fetch(ctx, b") == 2
    assert code.count("YGZ_LAUNCH(") == 2 and "hipStreamSynchronize" not in code and "hipMemcpy" not in code
    # every lane's index is tested against the count before an array is read
    assert "if (i >= A.n_total) return;" in code and "if (i >= n) return;" in code
