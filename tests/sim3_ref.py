"""ctypes loader of tests/sim3_ref.c, the restatement of the loop detection's Sim3 solver (ygz_slam_amd/csrc/sim3.hip) that
tests/test_sim3_ref.py and tests/test_gpu_sim3.py hold ygz_hip_sim3_ransac against.  Test infrastructure: compiled with gcc into a temporary
directory the first time it is used, never imported by the package.  Also the seeded synthetic 3D-3D scenes of the tests."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


class SrResult(ctypes.Structure):
    """the result block of sim3_ref.c (the layout of ygz_sim3_result, include/ygz_hip.h)"""
    _fields_ = [("S12", ctypes.c_double * 8), ("S21", ctypes.c_double * 8), ("chi2_ransac", ctypes.c_double), ("chi2_refined", ctypes.c_double),
                ("success", ctypes.c_int32), ("n_hypotheses", ctypes.c_int32), ("best_sample", ctypes.c_int32), ("n_inliers", ctypes.c_int32),
                ("n_refined", ctypes.c_int32), ("lm_iterations", ctypes.c_int32)]


class SrParams(ctypes.Structure):
    _fields_ = [("max_iter", ctypes.c_int), ("chi2", ctypes.c_double), ("min_inliers", ctypes.c_int), ("chi2_refine", ctypes.c_double),
                ("iters_first", ctypes.c_int), ("iters_more", ctypes.c_int), ("iters_again", ctypes.c_int), ("fix_scale", ctypes.c_int)]


# ORB-SLAM2 LoopClosing::ComputeSim3 / Optimizer::OptimizeSim3
DEFAULTS = dict(max_iter=300, chi2=9.210, min_inliers=20, chi2_refine=10.0, iters_first=5, iters_more=10, iters_again=5, fix_scale=0)


def result_dict(r):
    d = {}
    for name, ty in r._fields_:
        v = getattr(r, name)
        d[name] = np.array(v[:]) if hasattr(ty, "_length_") else v
    return d


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="sim3_ref_")
        so = os.path.join(d, "libsim3_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "sim3_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        _lib.sr_sigma2.restype = ctypes.c_double
    return _lib


def _d(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(shape) if shape else a


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(**kw):
    p = SrParams()
    for k, v in dict(DEFAULTS, **kw).items():
        setattr(p, k, v)
    return p


def sample_sets(n, max_iter=300):
    s = np.zeros((max_iter, 3), np.int32)
    lib().sr_sample_sets(n, max_iter, _p(s, ctypes.c_int32))
    return s


def horn(X1, X2, fix_scale=False):
    """-> (ok, S12 [8], S21 [8]) from n correspondences"""
    X1, X2 = _d(X1, (-1, 3)), _d(X2, (-1, 3))
    S12, S21 = np.zeros(8), np.zeros(8)
    ok = lib().sr_horn(_p(X1), _p(X2), len(X1), int(fix_scale), _p(S12), _p(S21))
    return ok, S12, S21


def solve3(X1, X2, fix_scale=False):
    h = np.zeros(16)
    ok = lib().sr_solve3(_p(_d(X1, (3, 3))), _p(_d(X2, (3, 3))), int(fix_scale), _p(h))
    return ok, h[:8], h[8:]


def apply_delta(S, x):
    out = np.zeros(8)
    ok = lib().sr_apply_delta(_p(_d(S)), _p(_d(x)), _p(out))
    return ok, out


def pair_terms(S, X1, X2, u1, u2, l1, l2, K4, fix_scale=False):
    """-> dict(e12, e21 [2], J12, J21 [2][7], c12, c21)"""
    e12, e21, J12, J21 = np.zeros(2), np.zeros(2), np.zeros((2, 7)), np.zeros((2, 7))
    c12, c21 = ctypes.c_double(), ctypes.c_double()
    lib().sr_pair_terms(_p(_d(S)), _p(_d(X1)), _p(_d(X2)), _p(_d(u1)), _p(_d(u2)), int(l1), int(l2), _p(_d(K4)), int(fix_scale), _p(e12), _p(e21),
                        _p(J12), _p(J21), ctypes.byref(c12), ctypes.byref(c21))
    return dict(e12=e12, e21=e21, J12=J12, J21=J21, c12=c12.value, c21=c21.value)


def hypotheses(sc, sets, chi2=9.210, fix_scale=False):
    X1, X2, u1, u2, lv = _d(sc["X1"]), _d(sc["X2"]), _d(sc["px1"]), _d(sc["px2"]), _i(sc["levels"])
    sets = _i(sets)
    n, it = len(X1), len(sets)
    hyp, val, cnt = np.zeros((it, 16)), np.zeros(it, np.int32), np.zeros(it, np.int32)
    lib().sr_hypotheses(_p(X1), _p(X2), _p(u1), _p(u2), _p(lv, ctypes.c_int32), n, _p(_d(sc["K4"])), _p(sets, ctypes.c_int32), it,
                        ctypes.c_double(chi2), int(fix_scale), _p(hyp), _p(val, ctypes.c_int32), _p(cnt, ctypes.c_int32))
    return dict(hyps=hyp, valid=val, counts=cnt)


def ransac(sc, **kw):
    """the whole call for one problem: result dict, mask [n] (bit 0 RANSAC inlier, bit 1 refined inlier), hyps, valid, counts, sets"""
    p = params(**kw)
    X1, X2, u1, u2, lv = _d(sc["X1"]), _d(sc["X2"]), _d(sc["px1"]), _d(sc["px2"]), _i(sc["levels"])
    n, it = len(X1), p.max_iter
    sets = np.zeros((it, 3), np.int32)
    hyp, val, cnt = np.zeros((it, 16)), np.zeros(it, np.int32), np.zeros(it, np.int32)
    r, mask = SrResult(), np.zeros(n, np.uint8)
    lib().sr_ransac(_p(X1), _p(X2), _p(u1), _p(u2), _p(lv, ctypes.c_int32), n, _p(_d(sc["K4"])), ctypes.byref(p), _p(sets, ctypes.c_int32), _p(hyp),
                    _p(val, ctypes.c_int32), _p(cnt, ctypes.c_int32), ctypes.byref(r), _p(mask, ctypes.c_uint8))
    return dict(result=result_dict(r), mask=mask, hyps=hyp, valid=val, counts=cnt, sets=sets)


# ---- Sim3 in numpy, and seeded synthetic 3D-3D scenes -------------------------------------------------------------------------------
K4_DEFAULT = np.array([520.9, 521.0, 325.1, 249.7], np.float32).astype(np.float64)     # config/default.yaml:32-35 (float intrinsics)


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-3:
        return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
    q = np.zeros(4)
    q[i] = t / 2
    q[3] = (R[k, j] - R[j, k]) / (2 * t)
    q[j] = (R[j, i] + R[i, j]) / (2 * t)
    q[k] = (R[k, i] + R[i, k]) / (2 * t)
    return q if q[3] >= 0 else -q


def act(S, X):
    return S[7] * (np.asarray(X) @ quat_to_R(S[:4]).T) + S[4:7]


def rot(axis, deg):
    a = np.asarray(axis, float); a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def project(K4, P):
    return np.stack([K4[0] * P[:, 0] / P[:, 2] + K4[2], K4[1] * P[:, 1] / P[:, 2] + K4[3]], 1)


def random_sim3(rng, scale=(0.5, 2.0), deg=(2, 30), t=0.3):
    R = rot(rng.normal(size=3), rng.uniform(*deg))
    return np.concatenate([R_to_quat(R), rng.uniform(-t, t, 3), [rng.uniform(*scale)]])


def scene(n, seed, noise=0.5, outliers=0.3, K4=K4_DEFAULT, w=640, h=480, fix_scale=False, max_level=3):
    """n points seen by camera 1 (X1, depths 2-6 m) and by camera 2 (X2 = S21 X1) with S12 a random Sim3 (s = 1 when fix_scale); pixels of
    both with noise sigma `noise` scaled by 2^level; a fraction `outliers` of the pairs gets X2 of another point"""
    rng = np.random.default_rng(seed)
    S12 = random_sim3(rng, scale=(1.0, 1.0) if fix_scale else (0.6, 1.6), deg=(2, 15), t=0.15)
    u = rng.uniform(20, w - 20, n); v = rng.uniform(20, h - 20, n)
    z = rng.uniform(2, 6, n)
    X1 = np.stack([(u - K4[0 + 2]) / K4[0] * z, (v - K4[3]) / K4[1] * z, z], 1)
    R, t, s = quat_to_R(S12[:4]), S12[4:7], S12[7]
    X2 = ((X1 - t) @ R) / s                                          # S12 X2 = X1
    levels = rng.integers(0, max_level + 1, (n, 2)).astype(np.int32)
    sig = 2.0 ** levels
    px1 = project(K4, X1) + rng.normal(0, 1, (n, 2)) * noise * sig[:, :1]
    px2 = project(K4, X2) + rng.normal(0, 1, (n, 2)) * noise * sig[:, 1:]
    k = int(round(outliers * n))
    out = np.zeros(n, bool)
    if k:
        idx = rng.choice(n, k, replace=False)
        perm = rng.permutation(idx)
        X2 = X2.copy(); px2 = px2.copy()
        X2[idx] = X2[perm] + rng.normal(0, 0.3, (k, 3)) * (perm == idx)[:, None]
        px2[idx] = px2[perm] + rng.uniform(30, 80, (k, 2)) * (perm == idx)[:, None]
        out[idx] = True
    return dict(X1=X1, X2=X2, px1=px1, px2=px2, levels=levels, K4=np.asarray(K4, float), S12=S12, outlier=out)
