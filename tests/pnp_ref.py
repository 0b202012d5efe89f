"""ctypes loader of tests/pnp_ref.c, the restatement of the relocalisation pose solver (ygz_slam_amd/csrc/pnp.hip) that
tests/test_pnp_ref.py and tests/test_gpu_pnp.py hold ygz_hip_pnp_ransac against.  Test infrastructure: compiled with gcc into a temporary
directory the first time it is used, never imported by the package.  Also the seeded synthetic 2D-3D scenes of the tests."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class PrResult(ctypes.Structure):
    """the result block of pnp_ref.c (the layout of ygz_pnp_result, include/ygz_hip.h)"""
    _fields_ = [("R", ctypes.c_double * 9), ("t", ctypes.c_double * 3), ("T_cw", ctypes.c_double * 7), ("success", ctypes.c_int32),
                ("n_inliers", ctypes.c_int32), ("best_sample", ctypes.c_int32), ("best_solution", ctypes.c_int32),
                ("n_hypotheses", ctypes.c_int32)]


def result_dict(r):
    d = {}
    for name, ty in r._fields_:
        v = getattr(r, name)
        d[name] = np.array(v[:]) if hasattr(ty, "_length_") else v
    return d


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="pnp_ref_")
        so = os.path.join(d, "libpnp_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "pnp_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        _lib.pr_cubic_root.restype = ctypes.c_double
        _lib.pr_cubic_root.argtypes = [ctypes.c_double] * 3
    return _lib


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


DEFAULTS = dict(max_iter=300, chi2=5.991, min_inliers=10)        # ORB-SLAM2 Tracking::Relocalization


def sample_sets(n, max_iter=300):
    s = np.zeros((max_iter, 3), np.int32)
    lib().pr_sample_sets(n, max_iter, _p(s, ctypes.c_int32))
    return s


def cubic_root(b, c, d):
    return lib().pr_cubic_root(b, c, d)


def p3p(pw3, px3, K4):
    """-> (count, solutions [count][12]: R row-major, t)"""
    sol = np.zeros((4, 12))
    n = lib().pr_p3p(_p(_d(pw3)), _p(_d(px3)), _p(_d(K4)), _p(sol))
    return n, sol[:n]


def hypotheses(pw, px, K4, sets, chi2=5.991):
    pw, px, sets = _d(pw), _d(px), np.ascontiguousarray(sets, np.int32)
    n, it = len(pw), len(sets)
    sol, ns, cnt = np.zeros((it, 4, 12)), np.zeros(it, np.int32), np.zeros((it, 4), np.int32)
    lib().pr_hypotheses(_p(pw), _p(px), n, _p(_d(K4)), _p(sets, ctypes.c_int32), it, ctypes.c_double(chi2), _p(sol), _p(ns, ctypes.c_int32),
                        _p(cnt, ctypes.c_int32))
    return dict(solutions=sol, n_solutions=ns, counts=cnt)


def ransac(pw, px, K4, **kw):
    o = dict(DEFAULTS, **kw)
    pw, px = _d(pw), _d(px)
    n, it = len(pw), int(o["max_iter"])
    sets = np.zeros((it, 3), np.int32)
    sol, ns, cnt = np.zeros((it, 4, 12)), np.zeros(it, np.int32), np.zeros((it, 4), np.int32)
    r, inl = PrResult(), np.zeros(n, np.uint8)
    lib().pr_ransac(_p(pw), _p(px), n, _p(_d(K4)), it, ctypes.c_double(o["chi2"]), int(o["min_inliers"]), _p(sets, ctypes.c_int32), _p(sol),
                    _p(ns, ctypes.c_int32), _p(cnt, ctypes.c_int32), ctypes.byref(r), _p(inl, ctypes.c_uint8))
    return dict(result=result_dict(r), inliers=inl.astype(bool), solutions=sol, n_solutions=ns, counts=cnt, sets=sets)


# ---- seeded synthetic 2D-3D scenes ------------------------------------------------------------------------------------------------
K4_DEFAULT = np.array([520.9, 521.0, 325.1, 249.7], np.float32).astype(np.float64)     # config/default.yaml:32-35 (float intrinsics)


def rot(axis, deg):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(K4, P):
    return np.stack([K4[0] * P[:, 0] / P[:, 2] + K4[2], K4[1] * P[:, 1] / P[:, 2] + K4[3]], 1)


def scene(n, seed, planar=False, noise=0.0, outliers=0.0, K4=K4_DEFAULT, w=640, h=480):
    """n world points seen by a camera of known pose T_cw = (R, t): spread over the image at depths 2-6 m, or on the world plane Z = 2
    (the map of synth.py) when planar; pixel noise sigma `noise`; a fraction `outliers` replaced by random pixels."""
    rng = np.random.default_rng(seed)
    R = rot(rng.normal(size=3), rng.uniform(2, 25))
    t = rng.uniform(-0.3, 0.3, 3)
    u = rng.uniform(20, w - 20, n); v = rng.uniform(20, h - 20, n)
    ray = np.stack([(u - K4[2]) / K4[0], (v - K4[3]) / K4[1], np.ones(n)], 1)          # camera frame, z = 1
    if planar:
        # world point = R^T (Pc - t) with Z_w = 2: the depth along each ray that reaches the plane
        Rt = R.T
        c = -Rt @ t                                                                        # camera centre in the world
        dw = ray @ Rt.T                                                                    # ray directions in the world
        s = (2.0 - c[2]) / dw[:, 2]
        Pw = c + dw * s[:, None]
        keep = s > 0
        assert keep.all()
    else:
        z = rng.uniform(2, 6, n)
        Pc = ray * z[:, None]
        Pw = (Pc - t) @ R
    Pc = Pw @ R.T + t
    px = project(K4, Pc) + (rng.normal(0, noise, (n, 2)) if noise > 0 else 0.0)
    k = int(round(outliers * n))
    out = np.zeros(n, bool)
    if k:
        idx = rng.choice(n, k, replace=False)
        px[idx] = np.stack([rng.uniform(0, w, k), rng.uniform(0, h, k)], 1)
        out[idx] = True
    return dict(pw=Pw, px=px, R=R, t=t, K4=np.asarray(K4, float), outlier=out)
