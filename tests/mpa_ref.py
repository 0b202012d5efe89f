"""ctypes loader of tests/mpa_ref.c, the restatement of the map-point attributes (ygz_slam_amd/csrc/mpa.hip) that
tests/test_mpa_ref.py holds to a numpy witness and to Matcher::PointAttributes' formula in plain floats, and tests/test_gpu_mpa.py holds
ygz_hip_map_point_attributes against.  Test infrastructure: compiled with gcc (-ffp-contract=off) into a temporary directory the first time it
is used, never imported by the package.  Also the maps both tests share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

MAX_POINTS, MAX_KEYFRAMES, MAX_OBS, MAX_OBS_PER_POINT, MAX_LEVEL = 1048576, 4096, 1048576, 256, 30
OUTPUTS = ("dmax", "normal", "state")


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="mpa_ref_")
        so = os.path.join(d, "libmpa_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "mpa_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def arrays(m):
    """the arrays of a map in the ABI's types (obs_kf and obs_level of at least one element)"""
    one = lambda a: a if len(a) else np.zeros(1, np.int32)
    return dict(center=np.ascontiguousarray(m["center"], np.float64).reshape(-1, 3), pw=np.ascontiguousarray(m["pw"], np.float64).reshape(-1, 3),
                off=np.ascontiguousarray(m["off"], np.int32), kf=one(np.ascontiguousarray(m["kf"], np.int32)),
                level=one(np.ascontiguousarray(m["level"], np.int32)))


def attributes(m):
    """mr_attributes on a map: dict of dmax [P], normal [P, 3], state [P]"""
    a = arrays(m)
    P = len(a["pw"])
    o = dict(dmax=np.full(P, -7.0), normal=np.full((P, 3), -7.0), state=np.full(P, -7, np.int32))
    rc = lib().mr_attributes(len(a["center"]), _p(a["center"], ctypes.c_double), P, _p(a["pw"], ctypes.c_double), _p(a["off"], ctypes.c_int32),
                             _p(a["kf"], ctypes.c_int32), _p(a["level"], ctypes.c_int32), _p(o["dmax"], ctypes.c_double),
                             _p(o["normal"], ctypes.c_double), _p(o["state"], ctypes.c_int32))
    assert rc == 0
    return o


def same(got, want):
    """every output on bits: doubles as uint64, the state exact"""
    for k in OUTPUTS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if k != "state":
            g, w = g.view(np.uint64), w.view(np.uint64)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:6]
            raise AssertionError((k, bad.tolist(), [got[k][tuple(b)] for b in bad], [want[k][tuple(b)] for b in bad]))


def make_map(K, rows, seed, levels=(-1, 0, 1, 2, 3, 7, 30)):
    """a map of len(rows) points with rows[p] rows each on K keyframes: centres in a 10 m box, points around them, obs_kf in any order and
    with repeats, the levels drawn from `levels`"""
    rng = np.random.default_rng(seed)
    rows = np.asarray(rows, np.int64)
    P, n = len(rows), int(rows.sum())
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return dict(center=rng.uniform(-5, 5, (K, 3)), pw=rng.uniform(-8, 8, (P, 3)) + [0, 0, 12.0], off=off,
                kf=rng.integers(0, K, n).astype(np.int32), level=rng.choice(np.asarray(levels, np.int32), n).astype(np.int32))


def ragged_rows(P, seed, top=12):
    """row counts with 0, 1, 2, 255 and 256 among the first lanes of the first wavefront when P allows it"""
    rows = np.random.default_rng(seed).integers(0, top + 1, P)
    for i, v in enumerate((0, 256, 1, 255, 2, 256, 0)):
        if i < P:
            rows[i] = v
    return rows


def degenerate_map():
    """eight points on three keyframes: on a centre (d = 0); 1e-300 from a centre (q underflows to 0); coordinates of 1e155 (q overflows); a
    usable point beside them; a point whose SECOND row is on a centre; no row; the same keyframe three times; coordinates of 1e150, whose
    squares (1e300) still fit a double, so the point is usable.  (the map, the state of every point)"""
    center = np.array([[0.0, 0, 0], [1.0, 2, 3], [-4.0, 0.5, 2]])
    pw = np.array([[1.0, 2, 3], [1e-300, 0, 0], [1e155, -1e155, 1e155], [0.3, -0.2, 5.0], [-4.0, 0.5, 2], [2.0, 2, 2], [0.5, 0.25, 4.0],
                   [1e150, -1e150, 1e150]])
    rows = [[1, 0], [0], [0, 1], [0, 1, 2], [0, 2], [], [1, 1, 1], [0]]
    level = [[2, 0], [0], [3, 1], [7, 0, -1], [1, 0], [], [30, 0, 5], [0]]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return dict(center=center, pw=pw, off=off, kf=np.concatenate([np.array(r, np.int32) for r in rows]),
                level=np.concatenate([np.array(r, np.int32) for r in level])), [2, 2, 2, 1, 2, 0, 1, 1]
