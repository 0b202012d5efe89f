"""The keyframe-culling calls on the MI355X (ygz_hip_keyframe_redundancy, ygz_hip_cull_keyframes; ygz_slam_amd/csrc/cull.hip) against their
restatement tests/cull_ref.c, every output bit for bit, on the cases of tests/cull_ref.py: points of 0 to 5 observations, exactly th_obs - 1,
th_obs and th_obs + 1 other observers, levels on both sides of the slack, lists of 63 / 64 / 65 / 255 / 256 entries, 300 points that straddle
wavefronts and blocks, 1, 2, 130 and 4096 keyframes, keyframes without points, every point on keyframe 0; walks of 1, 64, 65 and K candidates,
shuffled subsets, candidates of 0, 1025 and 2500 observations, the ratio boundary, the order-dependence pair and the death cascade; refusals
through a live context."""
import ctypes

import numpy as np
import pytest

import cull_ref as cr

pytestmark = pytest.mark.gpu

COUNTS = cr.count_cases()
WALKS = cr.walk_cases()
WALK_KEYS = ["culled", "tracked", "redundant", "point_dead"]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """the restatement's answer for every case, computed once"""
    return (dict((k, cr.run_counts(v)) for k, v in COUNTS.items()), dict((k, cr.run_walk(v)) for k, v in WALKS.items()))


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_redundancy_equals_the_restatement(ctx, expected, name):
    got, ref = cr.run_counts(COUNTS[name], ctx.keyframe_redundancy), expected[0][name]
    for k in ["tracked", "redundant"]:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k
    if name == "hand_k5":
        assert got["tracked"].tolist() == cr.HAND["tracked"] and got["redundant"].tolist() == cr.HAND["redundant"]


@pytest.mark.parametrize("name", sorted(WALKS))
def test_walk_equals_the_restatement(ctx, expected, name):
    got, ref = cr.run_walk(WALKS[name], ctx.cull_keyframes), expected[1][name]
    for k in WALK_KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    if name in cr.EXPECTED_CULLED:
        assert got["culled"].tolist() == cr.EXPECTED_CULLED[name]


def test_repeated_calls_give_the_same_bits(ctx, expected):
    """integer atomics and one workgroup's walk: the arrival order does not show"""
    for _ in range(3):
        got = cr.run_counts(COUNTS["column0"], ctx.keyframe_redundancy)
        assert np.array_equal(got["tracked"], expected[0]["column0"]["tracked"])
        assert np.array_equal(got["redundant"], expected[0]["column0"]["redundant"])
    for name in ["cand_all", "big_first"]:
        for _ in range(3):
            got = cr.run_walk(WALKS[name], ctx.cull_keyframes)
            for k in WALK_KEYS:
                assert np.array_equal(got[k], expected[1][name][k]), (name, k)


def test_the_walk_with_one_candidate_is_the_counts_decision(ctx):
    for k in [3, 77, 129]:
        case = WALKS["one_kf%d" % k]
        walk, counts = cr.run_walk(case, ctx.cull_keyframes), cr.run_counts(case, ctx.keyframe_redundancy)
        assert walk["tracked"][0] == counts["tracked"][k] and walk["redundant"][0] == counts["redundant"][k]
        assert walk["culled"][0] == int(float(counts["redundant"][k]) > case["params"]["ratio"] * float(counts["tracked"][k]))
        assert walk["point_dead"].sum() == 0 or walk["culled"][0] == 1


def test_refusals_through_a_live_context(ctx, hip_lib):
    lib = hip_lib.load()
    hip_lib.cull_argtypes(lib)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    off, kf, lv = np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.zeros(2, np.int32)
    t, r, c = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    red = lambda off, kf, lv, K, prm=None: lib.ygz_hip_keyframe_redundancy(ctx._ctx, len(off) - 1, ip(off), ip(kf), ip(lv), K, prm, ip(t), ip(r))
    walk = lambda cand, K=2, prm=None: lib.ygz_hip_cull_keyframes(ctx._ctx, 1, ip(off), ip(kf), ip(lv), K, len(cand), ip(cand), prm, ip(c), ip(t), ip(r), None)
    assert red(off, kf, lv, 2) == hip_lib.OK and t.tolist() == [1, 1] and r.tolist() == [0, 0]
    assert red(off, np.array([1, 1], np.int32), lv, 2) == hip_lib.E_INVALID
    assert red(off, kf, np.array([0, 16], np.int32), 2) == hip_lib.E_INVALID
    assert red(off, kf, lv, 1) == hip_lib.E_INVALID
    assert red(off, kf, lv, hip_lib.CULL_MAX_KEYFRAMES + 1) == hip_lib.E_CAPACITY
    assert red(np.array([0, 257], np.int32), kf, lv, 2) == hip_lib.E_CAPACITY
    assert red(off, kf, lv, 2, ctypes.byref(hip_lib._cull_params(ratio=1.5))) == hip_lib.E_INVALID
    assert walk(np.array([1, 0], np.int32)) == hip_lib.OK and c.tolist() == [0, 0]
    assert walk(np.array([1, 1], np.int32)) == hip_lib.E_INVALID
    assert walk(np.array([2], np.int32)) == hip_lib.E_INVALID
    assert walk(np.array([0], np.int32), prm=ctypes.byref(hip_lib._cull_params(th_obs=0))) == hip_lib.E_INVALID
