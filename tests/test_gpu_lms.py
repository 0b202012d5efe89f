"""The local-map selection on the MI355X (ygz_hip_local_map_select; ygz_slam_amd/csrc/lms.hip) against its restatement tests/lms_ref.c, every
output bit for bit, on every case of tests/lms_ref.py: the hand-made map, frames without points, a point twice on a frame, bad points and bad
keyframes, the vote tie, voters around max_keyframes, the covisible rows (shared first entry, rows of -1, a bad first entry, a voter, none at
all), a point of two local keyframes, observers outside the list, max_points around the set's size, a shared (keyframe, feature), lists of
63 .. 256 observations, keyframes of 255 .. 257 features, 1, 2, 130 and 4096 keyframes, 1, 3 and 65 frames.  Optional outputs as NULL, every
refusal of the header's list through a live context with the outputs untouched, and a smaller problem after a larger one through the same
context."""
import ctypes

import numpy as np
import pytest

import lms_ref as lr

pytestmark = pytest.mark.gpu

CASES = lr.cases()


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """the restatement's answer for every case, computed once"""
    return dict((k, lr.select(v)) for k, v in CASES.items())


def device(ctx, case, outputs=None):
    return ctx.local_map_select(case["kf_bad"], case["cov"], case["off"], case["kf"], case["feat"], case["fr_off"], case["fr_pt"],
                                pt_bad=case["pt_bad"], outputs=outputs, **case["params"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_restatement(ctx, expected, name):
    got, ref = device(ctx, CASES[name]), expected[name]
    assert sorted(got) == sorted(lr.OUTPUTS)
    for k in lr.OUTPUTS:
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    if name == "hand":
        for k in lr.OUTPUTS:
            assert got[k].tolist() == lr.HAND_OUT[k], k


def test_optional_outputs_as_null(ctx, expected):
    for name in ["hand", "k130_frames3", "frame_without_points"]:
        ref = expected[name]
        got = device(ctx, CASES[name], outputs=())
        assert sorted(got) == ["local_kf", "n_local"]
        assert np.array_equal(got["n_local"], ref["n_local"]) and np.array_equal(got["local_kf"], ref["local_kf"])
        for only in ["votes", "local_pt", "fr_prior", "ref"]:
            got = device(ctx, CASES[name], outputs=(only,))
            assert sorted(got) == sorted({only, "local_kf", "n_local"})
            for k in got:
                assert np.array_equal(got[k], ref[k]), (name, only, k)


def test_a_smaller_problem_after_a_larger_one(ctx, expected):
    """the scratch block keeps the larger call's rank tables, counts and kept lists: none of it may show"""
    small = lr.smaller_case()
    ref = lr.select(small)
    for big in ["k4096", "k130_frames65"]:
        got = device(ctx, CASES[big])
        for k in lr.OUTPUTS:
            assert np.array_equal(got[k], expected[big][k]), (big, k)
        got = device(ctx, small)
        for k in lr.OUTPUTS:
            assert np.array_equal(got[k], ref[k]), (big, k)


def test_repeated_calls_give_the_same_bits(ctx, expected):
    for _ in range(3):
        got = device(ctx, CASES["k130_frames65"])
        for k in lr.OUTPUTS:
            assert np.array_equal(got[k], expected["k130_frames65"][k]), k


def test_refusals_through_a_live_context(ctx, hip_lib):
    lib = hip_lib.load()
    hip_lib.lms_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def params(**kw):
        p = hip_lib.LmsParams()
        lib.ygz_hip_default_lms_params(ctypes.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def call(K=2, C=1, kf_bad=(0, 0), cov=(1, 0), off=(0, 2, 3), kf=(0, 1, 1), feat=(0, 0, 1), pt_bad=None, fr_off=(0, 2), fr_pt=(0, 1), F=None, P=None,
             p=None, null=(), keep=False):
        a = dict(kf_bad=np.array(kf_bad, np.uint8), cov=np.array(cov, np.int32), off=np.array(off, np.int32), kf=np.array(kf, np.int32),
                 feat=np.array(feat, np.int32), fr_off=np.array(fr_off, np.int32), fr_pt=np.array(fr_pt, np.int32))
        F = len(fr_off) - 1 if F is None else F
        P = len(off) - 1 if P is None else P
        mp = 4 if p is None else max(1, min(int(p.max_points), 64))
        p = params(max_points=4) if p is None else p
        n = max(F, 1)
        out = [np.full(n * max(K, 1), 5, np.int32), np.full(n, 5, np.int32), np.full(n, 5, np.int32), np.full(n, 5, np.int32),
               np.full(n * max(K, 1), 5, np.int32), np.full(n, 5, np.int32), np.full(n, 5, np.int32), np.full(n * mp, 5, np.int32),
               np.full(max(len(a["fr_pt"]), 1), 5, np.int32)]
        arg = dict((k, bp(v) if k == "kf_bad" else ip(v)) for k, v in a.items())
        outs = [ip(o) for o in out]
        for k in null:
            if k in arg:
                arg[k] = None
            else:
                outs[lr.OUTPUTS.index(k)] = None
        pb = None if pt_bad is None else np.array(pt_bad, np.uint8)
        rc = lib.ygz_hip_local_map_select(ctx._ctx, K, arg["kf_bad"], C, arg["cov"], P, arg["off"], arg["kf"], arg["feat"],
                                          None if pb is None else bp(pb), F, arg["fr_off"], arg["fr_pt"], ctypes.byref(p), *outs)
        if not keep:
            assert rc != hip_lib.OK and all((o == 5).all() for o in out), rc                  # a refused call writes nothing
        return (rc, out) if keep else rc
    # 0: the call is a valid one
    rc, out = call(keep=True)
    assert rc == hip_lib.OK and out[3].tolist() == [2] and out[4].tolist() == [0, 1] and out[7].tolist() == [0, 1, -1, -1]
    # 1: nulls and counts
    for k in ("kf_bad", "off", "kf", "feat", "fr_off", "fr_pt", "n_local", "local_kf", "cov"):
        assert call(null=(k,)) == INV, k
    assert call(K=0) == INV and call(C=-1) == INV and call(P=0) == INV and call(F=0) == INV and call(F=-1) == INV
    # 2: capacities, before the parameters
    big = hip_lib.LMS_MAX_KEYFRAMES + 1
    assert call(K=big, kf_bad=[0] * big, cov=[-1] * big) == CAP and call(K=big, kf_bad=[0] * big, cov=[-1] * big, p=params(max_keyframes=0)) == CAP
    assert call(C=hip_lib.LMS_MAX_COV + 1, cov=[-1] * (2 * (hip_lib.LMS_MAX_COV + 1))) == CAP
    big = hip_lib.LMS_MAX_FRAMES + 1
    assert call(fr_off=[0] * (big + 1), fr_pt=[]) == CAP
    assert call(K=big, kf_bad=[0] * big, cov=[-1] * big, null=("n_local",)) == INV              # the nulls come before the capacities
    # 3: parameters
    for bad in (dict(max_keyframes=0), dict(max_keyframes=-1), dict(max_keyframes=hip_lib.LMS_MAX_KEYFRAMES + 1), dict(max_points=0), dict(max_points=-3)):
        assert call(p=params(**bad)) == INV, bad
    # 4: the products, before the offsets
    assert call(p=params(max_points=hip_lib.SLM_MAX_PAIRS + 1)) == CAP
    assert call(fr_off=[0] * 5, fr_pt=[], p=params(max_points=hip_lib.SLM_MAX_PAIRS // 4 + 1)) == CAP
    assert call(fr_off=[0] * 5, fr_pt=[], off=(1, 2, 3), p=params(max_points=hip_lib.SLM_MAX_PAIRS // 4 + 1)) == CAP
    # n_frames * n_keyframes above YGZ_COVIS_MAX_CELLS cannot be formed: the two limits of (2) multiply to exactly that bound
    assert hip_lib.LMS_MAX_KEYFRAMES * hip_lib.LMS_MAX_FRAMES == hip_lib.COVIS_MAX_CELLS
    # 5: offsets
    assert call(off=(1, 2, 3)) == INV and call(off=(0, 3, 2)) == INV and call(fr_off=(1, 2)) == INV and call(fr_off=(0, 2, 1), fr_pt=(0, 1)) == INV
    # 6: the sizes of the lists
    n = hip_lib.MAP_MAX_OBS_PER_POINT + 1
    assert call(K=n, kf_bad=[0] * n, cov=[-1] * n, off=(0, n), kf=list(range(n)), feat=[0] * n) == CAP
    assert call(K=n, kf_bad=[0] * n, cov=[-1] * n, off=(0, n), kf=[0] * n, feat=[0] * n) == CAP   # before the lists are read
    n = hip_lib.LMS_MAX_FEATURES + 1
    assert call(fr_off=(0, n), fr_pt=[0] * n) == CAP and call(fr_off=(0, n), fr_pt=[7] * n) == CAP
    # 7: indices
    assert call(kf=(0, 2, 1)) == INV and call(kf=(-1, 1, 1)) == INV and call(kf=(1, 1, 1)) == INV and call(kf=(1, 0, 1)) == INV
    assert call(feat=(0, -1, 1)) == INV and call(feat=(0, hip_lib.LMS_MAX_FEATURES, 1)) == INV
    assert call(cov=(2, 0)) == INV and call(cov=(1, -2)) == INV and call(fr_pt=(0, 2)) == INV and call(fr_pt=(-2, 1)) == INV
    # the limits themselves pass
    rc, out = call(feat=(0, hip_lib.LMS_MAX_FEATURES - 1, 1), cov=(-1, -1), fr_pt=(-1, 1), keep=True)
    assert rc == hip_lib.OK and out[3].tolist() == [1]
