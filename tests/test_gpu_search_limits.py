"""The crafted limit cases of tests/search_limit_cases.py on the MI355X: k_strack_search with the host claim walk of its entry point
(ygz_slam_amd/csrc/strack.hip) and k_lfuse_search (csrc/lfuse.hip).  Every case puts one input ON a limit of a rule of DESIGN.md sections
12, 25 and 26, or one np.nextafter step beyond it, with everything exact in FP64.  For every case, with its keypoints at index 0, 7, 8,
255 and 256 of 257 and its points at index 0, 63, 64 and 256 of 257: every output of the device is byte-equal to the restatement
(tests/strack_ref.c, tests/lfuse_ref.c; the comparison of check() in tests/test_gpu_strack.py), and the case's LITERAL expectation holds
on the device's output.  Every case runs alone, and once more as one of up to 64 problems of one call that share point sets: a limit must
not depend on the blockIdx.y that carries it.  Contexts of three and of five pyramid levels (the level ranges that poke out of the pyramid
need five).  No case is skipped and no comparison has a tolerance; tests/test_search_limit_cases.py shows on the CPU that the cases
separate every wrong variant of every rule."""
import numpy as np
import pytest

import lfuse_ref as lf
import search_limit_cases as slc
import strack_ref as st
from conftest import make_ctx

pytestmark = pytest.mark.gpu

NAMES = dict(strack=("match", "dist", "level", "reason", "outcome", "n_cand", "n_gated", "proj", "cand", "counts", "rot"),
             lfuse=("match", "dist", "pred_level", "reason", "n_gated", "counts"))


@pytest.fixture(scope="module")
def ctxs(hip_lib):
    made = {L: make_ctx(hip_lib, width=slc.W, height=slc.H, levels=L, max_frames=2, intrinsics=slc.KX) for L in (3, 5)}
    yield made
    for c in made.values():
        c.close()


def check(ctxs, case, sets, problems):
    """one call on the device and on the restatement: every output equal, byte for byte"""
    ctx, L, fields = ctxs[case.params["L"]], case.params["L"], slc.fields_of(case)
    if case.kind == "strack":
        got, want = ctx.stereo_track_search(sets, problems, slc.KX, **fields), st.search(sets, problems, slc.KX, slc.W, slc.H, L, **fields)
        offsets = st.offsets(sets, problems)
    else:
        got, want = ctx.local_fuse_search(sets, problems, slc.KX, **fields), lf.search(sets, problems, slc.KX, slc.W, slc.H, L, **fields)
        offsets = lf.offsets(sets, problems)
    for k in NAMES[case.kind]:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), (case.name, k)
    assert np.array_equal(got["offsets"], offsets)
    return got


@pytest.mark.parametrize("kind", ["strack", "lfuse"])
def test_every_case_alone(ctxs, kind):
    cases = [c for c in slc.all_cases() if c.kind == kind]
    assert len(cases) >= 500 and {c.params["L"] for c in cases} == {3, 5}
    for c in cases:
        got = check(ctxs, c, c.sets, c.problems)
        assert slc.holds(c, got) == [], c.name


@pytest.mark.parametrize("kind", ["strack", "lfuse"])
def test_every_case_as_one_problem_of_many(ctxs, kind):
    cases = [c for c in slc.all_cases() if c.kind == kind]
    seen, largest = 0, 0
    for fam in slc.families(cases):
        for sets, problems, slots in slc.pack(fam):
            assert len(problems) <= 64 and len(sets) <= 8 and all(len(s["pt_desc"]) <= 257 for s in sets)
            got = check(ctxs, fam[0], sets, problems)
            for slot in slots:
                assert slc.holds(slot[0], slc.slot_outputs(got, got["offsets"], slot)) == [], slot[0].name
            seen += len(slots)
            largest = max(largest, len(problems))
    assert seen == len(cases) and largest == 64                        # no case is left out; a call of 64 problems occurs
