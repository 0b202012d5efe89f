"""The map-upkeep calls on the MI355X (ygz_hip_distinctive_descriptors, ygz_hip_covisibility; ygz_slam_amd/csrc/map.hip) against their
restatement tests/map_ref.c, every output bit for bit, on the cases of tests/map_ref.py: points of 0 to 5 observations, identical and
clustered descriptors (tied medians), 63 / 64 / 65 / 255 / 256 observations, 300 points of 1 to 12 observations that straddle wavefronts and
blocks; one and two keyframes, a hand-made case against literal numbers, 130 keyframes with every row and with a shuffled subset, 2000 points,
every point on keyframe 0 (one contended column), empty lists; refusals through a live context."""
import ctypes

import numpy as np
import pytest

import map_ref as mr

pytestmark = pytest.mark.gpu

DESC = mr.descriptor_cases()
WEIGHTS = mr.weight_cases()


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """the restatement's answer for every case, computed once"""
    return (dict((k, mr.distinctive(*v)) for k, v in DESC.items()), dict((k, mr.covisibility(*v)) for k, v in WEIGHTS.items()))


@pytest.mark.parametrize("name", sorted(DESC))
def test_distinctive_descriptors_equal_the_restatement(ctx, expected, name):
    off, desc = DESC[name]
    got, ref = ctx.distinctive_descriptors(off, desc), expected[0][name]
    for k in ["best", "median", "desc"]:
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("name", sorted(WEIGHTS))
def test_covisibility_equals_the_restatement(ctx, expected, name):
    off, kf, K, rows = WEIGHTS[name]
    got = ctx.covisibility(off, kf, K, rows)
    assert got.dtype == np.int32 and np.array_equal(got, expected[1][name])
    if name == "hand_k5":
        assert got.tolist() == mr.HAND_K5["weights"]


def test_repeated_calls_give_the_same_bits(ctx, expected):
    """atomicMin / atomicAdd on integers: the arrival order does not show"""
    off, desc = DESC["batch300"]
    for _ in range(3):
        got = ctx.distinctive_descriptors(off, desc)
        assert np.array_equal(got["best"], expected[0]["batch300"]["best"])
    off, kf, K, rows = WEIGHTS["column0"]
    for _ in range(3):
        assert np.array_equal(ctx.covisibility(off, kf, K, rows), expected[1]["column0"])


def test_refusals_through_a_live_context(ctx, hip_lib):
    lib = hip_lib.load()
    hip_lib.map_argtypes(lib)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    off, desc = np.array([0, 257], np.int32), np.zeros((257, 32), np.uint8)
    best = np.zeros(1, np.int32)
    assert lib.ygz_hip_distinctive_descriptors(ctx._ctx, 1, ip(off), bp(desc), ip(best), None, None) == hip_lib.E_CAPACITY
    assert lib.ygz_hip_distinctive_descriptors(ctx._ctx, 1, ip(np.array([0, -1], np.int32)), bp(desc), ip(best), None, None) == hip_lib.E_INVALID
    off, kf, rows, w = np.array([0, 2], np.int32), np.array([1, 1], np.int32), np.array([0], np.int32), np.zeros((1, 2), np.int32)
    assert lib.ygz_hip_covisibility(ctx._ctx, 1, ip(off), ip(kf), 2, 1, ip(rows), ip(w)) == hip_lib.E_INVALID
