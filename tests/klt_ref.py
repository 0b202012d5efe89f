"""ctypes loader of tests/klt_ref.c, the restatement of the pyramidal LK tracker (ygz_slam_amd/csrc/klt.hip) that tests/test_klt_ref.py pins to
the oracle and to the two recorded fixtures, and that tests/test_gpu_klt_ref.py holds ygz_hip_klt_track and ygz_hip_track_klt against, bit for
bit.  Test infrastructure: compiled with gcc into a temporary directory the first time it is used, never imported by the package.

The pyramid levels come from the oracle's pyr_down; the stop rule, the frames, Scharr and the tracker are the C side's.  `order` selects how the
five float sums of an evaluation are added: 0 as oracle/klt.c, 1 as k_klt3 (win 21), 2 as k_klt<false> (win 3..20); see klt_ref.c."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEVELS = 8
NOT_RUN, REF_OUT, EIG_FAIL, GUESS_OUT, CONVERGED, OSCILLATION, MAX_ITER, ERR_OUT = range(8)
EXIT_NAMES = ["not run", "reference window outside", "eigenvalue or determinant test failed", "guess window left the image",
              "converged by eps", "oscillation exit", "max_iter exhausted", "error window outside"]
EXITS = (REF_OUT, EIG_FAIL, GUESS_OUT, CONVERGED, OSCILLATION, MAX_ITER, ERR_OUT)
COARSE_EXITS = (REF_OUT, EIG_FAIL, GUESS_OUT, CONVERGED, OSCILLATION, MAX_ITER)          # the error is level 0's
DEFAULTS = dict(win=21, max_level=4, max_iter=30, eps=0.001, min_eig_threshold=1e-4, use_initial_flow=1)
_lib = None


class KrParams(ctypes.Structure):
    """kr_params of klt_ref.c (the layout of ygz_klt_params, include/ygz_hip.h, and of the oracle's yo_klt_params)"""
    _fields_ = [("win", ctypes.c_int), ("max_level", ctypes.c_int), ("max_iter", ctypes.c_int), ("eps", ctypes.c_double),
                ("min_eig_threshold", ctypes.c_double), ("use_initial_flow", ctypes.c_int)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="klt_ref_")
        so = os.path.join(d, "libklt_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "klt_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(**kw):
    p = KrParams()
    for k, v in dict(DEFAULTS, **kw).items():
        setattr(p, k, v)
    return p


def fill(prm, **kw):
    """the same fields on another binding's parameter struct (the oracle's, the library's)"""
    for k, v in dict(DEFAULTS, **kw).items():
        setattr(prm, k, v)
    return prm


def device_order(win):
    """the order of the kernel that ygz_launch_klt starts for this window"""
    return 1 if win == 21 else 2


def levels_used(w, h, **kw):
    p = params(**kw)
    return lib().kr_levels(w, h, p.win, p.max_level) + 1


def pyramid(oracle, img):
    """every level the tracker can ask for (at most MAX_LEVELS; a level is only used while it exceeds the smallest window, 3)"""
    lv = [np.ascontiguousarray(img, np.uint8)]
    while len(lv) < MAX_LEVELS and min((lv[-1].shape[0] + 1) // 2, (lv[-1].shape[1] + 1) // 2) > 3:
        lv.append(oracle.pyr_down(lv[-1]))
    return lv


def track(prev_lv, next_lv, pts, init, order, **kw):
    """dict(pts [n][2] f32, status [n] u8, err [n] f32, exit [n][8] i32, iters [n][8] i32, min_eig [n][8] f32, max_sum [n] f64, levels)"""
    p = params(**kw)
    pp = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    out = np.ascontiguousarray(init, np.float32).reshape(-1, 2).copy()
    n = len(pp)
    assert out.shape == pp.shape and len(prev_lv) == len(next_lv)
    st, err = np.zeros(n, np.uint8), np.zeros(n, np.float32)
    ex, it = np.zeros((n, MAX_LEVELS), np.int32), np.zeros((n, MAX_LEVELS), np.int32)
    me, ms = np.zeros((n, MAX_LEVELS), np.float32), np.zeros(n, np.float64)
    L = len(prev_lv)
    pa = (ctypes.POINTER(ctypes.c_uint8) * L)(*[_p(a, ctypes.c_uint8) for a in prev_lv])
    na = (ctypes.POINTER(ctypes.c_uint8) * L)(*[_p(a, ctypes.c_uint8) for a in next_lv])
    for a, b in zip(prev_lv, next_lv):
        assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.flags["C_CONTIGUOUS"] and b.flags["C_CONTIGUOUS"]
    lw = np.array([a.shape[1] for a in prev_lv], np.int32)
    lh = np.array([a.shape[0] for a in prev_lv], np.int32)
    rc = lib().kr_track(pa, na, _p(lw, ctypes.c_int), _p(lh, ctypes.c_int), L, _p(pp, ctypes.c_float), _p(out, ctypes.c_float), n,
                        ctypes.byref(p), int(order), _p(st, ctypes.c_uint8), _p(err, ctypes.c_float), _p(ex, ctypes.c_int32),
                        _p(it, ctypes.c_int32), _p(me, ctypes.c_float), _p(ms, ctypes.c_double))
    if rc != 0:
        raise RuntimeError("kr_track: %d (-1 invalid, -2 too few levels, -3 an int32 lane sum overflowed)" % rc)
    return dict(pts=out, status=st, err=err, exit=ex, iters=it, min_eig=me, max_sum=ms,
                levels=lib().kr_levels(int(lw[0]), int(lh[0]), p.win, p.max_level) + 1)


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def diff_report(tag, got, ref):
    """what an equality-of-bytes assertion prints: the points whose pts, status or err differ"""
    bad = np.flatnonzero(np.any(got[0].view(np.uint32).reshape(-1, 2) != ref[0].view(np.uint32).reshape(-1, 2), axis=1)
                         | (got[1] != ref[1]) | (got[2].view(np.uint32) != ref[2].view(np.uint32)))
    lines = ["%s: %d of %d points differ" % (tag, len(bad), len(ref[1]))]
    for i in bad[:8]:
        lines.append("  point %d: got %r %d %r, want %r %d %r" % (i, got[0][i].tolist(), got[1][i], float(got[2][i]),
                                                                   ref[0][i].tolist(), ref[1][i], float(ref[2][i])))
    return "\n".join(lines)
