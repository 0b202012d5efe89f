"""ctypes loader of tests/init_ref.c, the restatement of the reference's monocular Initializer (src/Algorithm/Initializer.cpp) that
tests/test_init_ref.py and tests/test_gpu_initializer.py hold ygz_hip_initialize against.  Test infrastructure: compiled with gcc into a
temporary directory the first time it is used, never imported by the package.  Also the seeded synthetic two-view scenes of the tests."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class IrResult(ctypes.Structure):
    """the result block of init_ref.c (the layout of ygz_init_result, include/ygz_hip.h)"""
    _fields_ = [("H21", ctypes.c_double * 9), ("F21", ctypes.c_double * 9), ("R21", ctypes.c_double * 9), ("t21", ctypes.c_double * 3),
                ("T21", ctypes.c_double * 7), ("parallax", ctypes.c_double), ("score_h", ctypes.c_float), ("score_f", ctypes.c_float),
                ("rh", ctypes.c_float), ("success", ctypes.c_int32), ("model", ctypes.c_int32), ("best_h", ctypes.c_int32),
                ("best_f", ctypes.c_int32), ("n_inliers", ctypes.c_int32), ("solution", ctypes.c_int32), ("n_good", ctypes.c_int32),
                ("second_good", ctypes.c_int32), ("similar", ctypes.c_int32), ("n_triangulated", ctypes.c_int32)]


def result_dict(r):
    d = {}
    for name, ty in r._fields_:
        v = getattr(r, name)
        d[name] = np.array(v[:]) if hasattr(ty, "_length_") else v
    return d


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="init_ref_")
        so = os.path.join(d, "libinit_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "init_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
    return _lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def sample_sets(n, max_iter=200):
    s = np.zeros((max_iter, 8), np.int32)
    lib().ir_sample_sets(n, max_iter, _p(s, ctypes.c_int32))
    return s


def null_vector(A):
    A = _d(A).copy()
    m, n = A.shape
    V = np.zeros((n, n)); x = np.zeros(n)
    lib().ir_null_vector(_p(A), m, n, _p(V), _p(x))
    return x


def svd3(A):
    U, s, V = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3))
    lib().ir_svd3(_p(_d(A)), _p(U), _p(s), _p(V))
    return U, s, V


def quat_from_matrix(R):
    q = np.zeros(4)
    lib().ir_quat_from_matrix(_p(_d(R)), _p(q))
    return q


def decompose_e(E):
    R1, R2, t = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3)
    lib().ir_decompose_e(_p(_d(E)), _p(R1), _p(R2), _p(t))
    return R1, R2, t


def h_solutions(H21, K4):
    K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
    Rs, ts = np.zeros((8, 3, 3)), np.zeros((8, 3))
    ok = lib().ir_h_solutions(_p(_d(H21)), _p(K), _p(Rs), _p(ts))
    return bool(ok), Rs, ts


def hypotheses(px1, px2, sets, sigma=2.0):
    px1, px2, sets = _d(px1), _d(px2), np.ascontiguousarray(sets, np.int32)
    n, it = len(px1), len(sets)
    H, F = np.zeros((it, 3, 3)), np.zeros((it, 3, 3))
    sh, sf = np.zeros(it, np.float32), np.zeros(it, np.float32)
    ih, jf = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    r = IrResult()
    lib().ir_hypotheses(_p(px1), _p(px2), n, _p(sets, ctypes.c_int32), it, ctypes.c_float(sigma), _p(H), _p(F), _p(sh, ctypes.c_float),
                        _p(sf, ctypes.c_float), ctypes.byref(r), _p(ih, ctypes.c_uint8), _p(jf, ctypes.c_uint8))
    return dict(H21=H, F21=F, score_h=sh, score_f=sf, inliers_h=ih.astype(bool), inliers_f=jf.astype(bool), result=result_dict(r))


DEFAULTS = dict(sigma=2.0, sigma2=4.0, max_iter=200, min_parallax=1.0, min_triangulated=8, good_point_ratio_h=0.9)   # Initializer.h Option


def reconstruct(px1, px2, K4, model, M, inliers, **kw):
    o = dict(DEFAULTS, **kw)
    px1, px2 = _d(px1), _d(px2)
    n = len(px1)
    inl = np.ascontiguousarray(inliers, np.uint8)
    p3d, tri = np.zeros((n, 3)), np.zeros(n, np.uint8)
    r = IrResult()
    lib().ir_reconstruct(_p(px1), _p(px2), n, _p(_d(K4)), int(model), _p(_d(M)), _p(inl, ctypes.c_uint8), ctypes.c_float(o["sigma2"]),
                         ctypes.c_double(o["min_parallax"]), int(o["min_triangulated"]), ctypes.c_double(o["good_point_ratio_h"]),
                         ctypes.byref(r), _p(p3d), _p(tri, ctypes.c_uint8))
    return dict(result=result_dict(r), pts3d=p3d, triangulated=tri.astype(bool))


def initialize(px1, px2, K4, **kw):
    o = dict(DEFAULTS, **kw)
    px1, px2 = _d(px1), _d(px2)
    n = len(px1)
    p3d, tri = np.zeros((n, 3)), np.zeros(n, np.uint8)
    r = IrResult()
    lib().ir_initialize(_p(px1), _p(px2), n, _p(_d(K4)), ctypes.c_float(o["sigma"]), ctypes.c_float(o["sigma2"]), int(o["max_iter"]),
                        ctypes.c_double(o["min_parallax"]), int(o["min_triangulated"]), ctypes.c_double(o["good_point_ratio_h"]),
                        ctypes.byref(r), _p(p3d), _p(tri, ctypes.c_uint8))
    return dict(result=result_dict(r), pts3d=p3d, triangulated=tri.astype(bool))


# ---- seeded synthetic two-view scenes -------------------------------------------------------------------------------------------
K4_DEFAULT = np.array([520.9, 521.0, 325.1, 249.7], np.float32).astype(np.float64)     # config/default.yaml:32-35 (PinholeCamera's float intrinsics)
K4_CONFIG = K4_DEFAULT


def rot(axis, deg):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(K4, P):
    return np.stack([K4[0] * P[:, 0] / P[:, 2] + K4[2], K4[1] * P[:, 1] / P[:, 2] + K4[3]], 1)


def scene(n, seed, planar=False, noise=0.5, outliers=0.0, R=None, t=None, K4=K4_DEFAULT):
    """n landmarks in front of camera 1 (depth 2-6 m, or the plane z = 4 when planar), seen by camera 2 = (R, t) (x2 = R x1 + t);
    pixel noise sigma `noise`, a fraction `outliers` of the matches replaced by random pixels in image 2."""
    rng = np.random.default_rng(seed)
    R = rot([0.2, 1.0, 0.1], 3.0) if R is None else R
    t = np.array([0.3, 0.02, 0.05]) if t is None else np.asarray(t, float)
    z = np.full(n, 4.0) if planar else rng.uniform(2, 6, n)
    u = rng.uniform(40, 600, n); v = rng.uniform(40, 440, n)
    P1 = np.stack([(u - K4[2]) / K4[0] * z, (v - K4[3]) / K4[1] * z, z], 1)
    P2 = P1 @ R.T + t
    px1 = project(K4, P1) + rng.normal(0, noise, (n, 2))
    px2 = project(K4, P2) + rng.normal(0, noise, (n, 2))
    k = int(round(outliers * n))
    if k:
        idx = rng.choice(n, k, replace=False)
        px2[idx] = np.stack([rng.uniform(0, 640, k), rng.uniform(0, 480, k)], 1)
    return dict(px1=px1, px2=px2, R=R, t=t, P1=P1, K4=np.asarray(K4, float))
