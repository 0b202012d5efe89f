"""ctypes loader of tests/smap_ref.c, the restatement of stereo map-point creation (ygz_slam_amd/csrc/smap.hip) that tests/test_smap_ref.py
holds to a numpy witness and tests/test_gpu_smap.py holds the device against.  Test infrastructure: compiled with gcc into a temporary
directory the first time it is used, never imported by the package.  Also the scenes the tests share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

OK, NO_METHOD, DEGENERATE, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE = range(9)
NONE, TRIANGULATE, UNPROJECT_1, UNPROJECT_2 = range(4)
K4 = (420.0, 421.5, 318.25, 243.125)          # the camera of the scenes: fx fy cx cy
WIDTH, HEIGHT = 640, 480
PARAM_FIELDS = ["baseline", "chi2_mono", "chi2_stereo", "cos_parallax_max", "ratio_factor", "th_depth", "min_close", "pad"]


class Params(ctypes.Structure):
    """sm_params = ygz_smap_params"""
    _fields_ = [(n, ctypes.c_double) for n in PARAM_FIELDS[:6]] + [("min_close", ctypes.c_int32), ("pad", ctypes.c_int32)]


class Problem(ctypes.Structure):
    """sm_problem = ygz_smap_problem"""
    _fields_ = [("T1", ctypes.c_double * 7), ("T2", ctypes.c_double * 7)] + \
               [(n, ctypes.POINTER(ctypes.c_double)) for n in ("px1", "px2", "ur1", "ur2", "depth1", "depth2")] + \
               [("level1", ctypes.POINTER(ctypes.c_int32)), ("level2", ctypes.POINTER(ctypes.c_int32)), ("n", ctypes.c_int)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="smap_ref_")
        so = os.path.join(d, "libsmap_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "smap_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        dp, ip, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
        _lib.sm_default_params.argtypes = [ctypes.POINTER(Params)]
        _lib.sm_default_params.restype = None
        _lib.sm_params_offset.argtypes = [ctypes.c_int]
        _lib.sm_cos_stereo.argtypes = [ctypes.c_double, ctypes.c_double]
        _lib.sm_cos_stereo.restype = ctypes.c_double
        _lib.sm_create.argtypes = [ctypes.POINTER(Problem), dp, ctypes.POINTER(Params), ip, ip, dp]
        _lib.sm_create.restype = None
        _lib.sm_keyframe_points.argtypes = [dp, dp, dp, bp, ctypes.c_int, dp, ctypes.POINTER(Params), ip, bp, dp, ip, ip]
        _lib.sm_keyframe_points.restype = None
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def default_params(**kw):
    p = Params()
    lib().sm_default_params(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def cos_stereo(d, b):
    return lib().sm_cos_stereo(float(d), float(b))


PROBLEM_ARRAYS = [("px1", np.float64), ("px2", np.float64), ("ur1", np.float64), ("ur2", np.float64), ("depth1", np.float64), ("depth2", np.float64),
                  ("level1", np.int32), ("level2", np.int32)]


def normalise(pb):
    """a problem (dict: T1, T2 and the eight arrays) with contiguous arrays of the right types"""
    out = dict(pb)
    out["T1"] = np.ascontiguousarray(pb["T1"], np.float64).reshape(7)
    out["T2"] = np.ascontiguousarray(pb["T2"], np.float64).reshape(7)
    for name, t in PROBLEM_ARRAYS:
        out[name] = np.ascontiguousarray(pb[name], t).reshape((-1, 2) if name.startswith("px") else (-1,))
    out["n"] = len(out["ur1"])
    return out


def c_problem(pb, cls=Problem):
    """the C struct of a normalised problem (the arrays must outlive it)"""
    s = cls()
    for k in range(7):
        s.T1[k], s.T2[k] = float(pb["T1"][k]), float(pb["T2"][k])
    for name, t in PROBLEM_ARRAYS:
        setattr(s, name, _p(pb[name], ctypes.c_double if t is np.float64 else ctypes.c_int32))
    s.n = int(pb["n"])
    return s


def create(pb, K4_=K4, params=None):
    """sm_create: (code [n], method [n], pos_world [n, 3])"""
    pb = normalise(pb)
    p = params if params is not None else default_params()
    n = pb["n"]
    code, method, pos = np.full(max(n, 1), -9, np.int32), np.full(max(n, 1), -9, np.int32), np.full((max(n, 1), 3), np.nan)
    k = np.ascontiguousarray(K4_, np.float64)
    s = c_problem(pb)
    lib().sm_create(ctypes.byref(s), _p(k, ctypes.c_double), ctypes.byref(p), _p(code, ctypes.c_int32), _p(method, ctypes.c_int32), _p(pos, ctypes.c_double))
    return code[:n], method[:n], pos[:n]


def keyframe_points(T, px, depth, has_point, K4_=K4, params=None):
    """sm_keyframe_points: dict(rank, selected, pos_world, n_depth, n_close)"""
    p = params if params is not None else default_params()
    T = np.ascontiguousarray(T, np.float64).reshape(7)
    px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
    depth = np.ascontiguousarray(depth, np.float64).reshape(-1)
    has = np.ascontiguousarray(has_point, np.uint8).reshape(-1)
    n = len(depth)
    m = max(n, 1)
    rank, sel, pos = np.full(m, -9, np.int32), np.full(m, 9, np.uint8), np.full((m, 3), np.nan)
    nd, nc = ctypes.c_int32(-1), ctypes.c_int32(-1)
    k = np.ascontiguousarray(K4_, np.float64)
    px_ = px if n else np.zeros((1, 2))
    depth_ = depth if n else np.zeros(1)
    has_ = has if n else np.zeros(1, np.uint8)
    lib().sm_keyframe_points(_p(T, ctypes.c_double), _p(px_, ctypes.c_double), _p(depth_, ctypes.c_double), _p(has_, ctypes.c_uint8), n,
                             _p(k, ctypes.c_double), ctypes.byref(p), _p(rank, ctypes.c_int32), _p(sel, ctypes.c_uint8), _p(pos, ctypes.c_double),
                             ctypes.byref(nd), ctypes.byref(nc))
    return dict(rank=rank[:n], selected=sel[:n], pos_world=pos[:n], n_depth=nd.value, n_close=nc.value)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------
def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def small_quat(rng, angle):
    a = rng.normal(size=3)
    a *= angle / np.linalg.norm(a)
    q = np.array([0.5 * a[0], 0.5 * a[1], 0.5 * a[2], 1.0])
    return q / np.linalg.norm(q)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def project(T, X, K4_=K4):
    """(px [n, 2], z [n]) of world points in the camera of pose T"""
    P = X @ quat_to_R(T[:4]).T + T[4:]
    z = P[:, 2]
    return np.stack([K4_[0] * P[:, 0] / z + K4_[2], K4_[1] * P[:, 1] / z + K4_[3]], 1), z


SCENE_KINDS = ["sideways", "forward", "mono", "wrong"]


def scene(kind, n, seed, baseline=0.1, mono_share=0.4, true_matches=False):
    """One problem of n pairs, seeded.  sideways: camera 2 is camera 1 moved 0.3 m along its x axis, points at 2-40 m; forward: moved 0.3 m along
    its z axis, points at 2-8 m, a quarter of them within 30 px of the epipole; mono: the sideways scene without stereo columns; wrong: the
    forward scene with matches that are wrong on purpose (pixels of camera 2 shifted by 3-30 px, depths off by 20 %).  Every pair carries random
    levels 0-2; about mono_share of the sides are mono (ur = -1); true_matches: level 0 on both sides (the matcher's own scale test passed).
    Pixel noise 0.3 px, disparity noise 0.2 px.  Also X [n, 3], the true points, and z1, z2, their true depths."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K4
    bf = fx * baseline
    q1 = small_quat(rng, 0.2)
    T1 = np.concatenate([q1, rng.normal(size=3) * 0.5])
    base = "sideways" if kind in ("sideways", "mono") else "forward"
    far = 40.0 if base == "sideways" else 8.0
    px1 = np.stack([rng.uniform(20, WIDTH - 20, n), rng.uniform(20, HEIGHT - 20, n)], 1)
    if base == "forward" and n:
        k = max(1, n // 4)                          # near the epipole, which is the principal point up to the small rotation
        r, a = rng.uniform(0.5, 30.0, k), rng.uniform(0, 2 * np.pi, k)
        px1[:k] = np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1)
    z1 = rng.uniform(2.0, far, n)
    R1 = quat_to_R(q1)
    Pc = np.stack([(px1[:, 0] - cx) / fx * z1, (px1[:, 1] - cy) / fy * z1, z1], 1)
    X = (Pc - T1[4:]) @ R1                          # R1^T (Pc - t1)
    # camera 2: T2 = D o T1 with D a small rotation and the translation that moves the centre by 0.3 m
    dq = small_quat(rng, 0.02)
    move = np.array([0.3, 0.0, 0.0]) if base == "sideways" else np.array([0.0, 0.0, 0.3])
    q2 = quat_mul(dq, q1)
    q2 /= np.linalg.norm(q2)
    t2 = quat_to_R(dq) @ (T1[4:] - move)
    T2 = np.concatenate([q2, t2])
    px2, z2 = project(T2, X)
    t_px1 = px1 + rng.normal(size=(n, 2)) * 0.3
    t_px2 = px2 + rng.normal(size=(n, 2)) * 0.3
    ur1 = t_px1[:, 0] - bf / z1 + rng.normal(size=n) * 0.2
    ur2 = t_px2[:, 0] - bf / np.where(z2 > 0.1, z2, 0.1) + rng.normal(size=n) * 0.2
    d1 = bf / np.maximum(t_px1[:, 0] - ur1, 1e-3)
    d2 = bf / np.maximum(t_px2[:, 0] - ur2, 1e-3)
    if kind == "wrong" and n:
        r, a = rng.uniform(3.0, 30.0, n), rng.uniform(0, 2 * np.pi, n)
        t_px2 = t_px2 + np.stack([r * np.cos(a), r * np.sin(a)], 1)
        d1, d2 = d1 * np.where(rng.random(n) < 0.5, 1.2, 0.8), d2 * np.where(rng.random(n) < 0.5, 1.2, 0.8)
    share = 1.0 if kind == "mono" else mono_share
    m1, m2 = rng.random(n) < share, rng.random(n) < share
    ur1, ur2 = np.where(m1 | (ur1 < 0), -1.0, ur1), np.where(m2 | (ur2 < 0), -1.0, ur2)
    l1, l2 = rng.integers(0, 3, n), rng.integers(0, 3, n)
    if true_matches:
        l1, l2 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    pb = normalise(dict(T1=T1, T2=T2, px1=t_px1, px2=t_px2, ur1=ur1, ur2=ur2, depth1=d1, depth2=d2, level1=l1, level2=l2))
    pb.update(X=X, z1=z1, z2=z2, kind=kind)
    return pb


def subset(pb, idx):
    """the pairs idx of a problem"""
    out = dict(pb)
    for name in [n for n, _ in PROBLEM_ARRAYS] + ["X", "z1", "z2"]:
        if name in pb:
            out[name] = np.ascontiguousarray(pb[name][idx])
    out["n"] = len(out["ur1"])
    return out


def edge_cases():
    """Two hand-made pairs for the codes no generic scene reaches, as (problem, K4, params, code, method):
     - x[3] == 0: two mono cameras side by side look at the same pixel (parallel rays) and cos_parallax_max = 2 lets them be triangulated; the third
       column of the system is exactly zero, so the Jacobi leaves e_3 as the null vector;
     - dist2 == 0: camera 2 (an exact quaternion, axes permuted) sits at (0, 0, 1) and the point un-projected from camera 1 is 1e-170 in front of
       it, so the square of the distance underflows while z2 > 0."""
    fx, fy, cx, cy = K4
    one = lambda v, t=np.float64: np.array([v], t)
    ident = [0, 0, 0, 1, 0, 0, 0]
    a = normalise(dict(T1=ident, T2=[0, 0, 0, 1, -1.0, 0, 0], px1=[[cx, cy]], px2=[[cx, cy]], ur1=one(-1.0), ur2=one(-1.0), depth1=one(0.0),
                       depth2=one(0.0), level1=one(0, np.int32), level2=one(0, np.int32)))
    kb = (fx, fy, cx, 0.0)
    b = normalise(dict(T1=ident, T2=[0.5, 0.5, 0.5, 0.5, -1.0, 0, 0], px1=[[cx, fy * 1e-170]], px2=[[cx - 1.0, 0.0]], ur1=one(cx - fx * 0.1), ur2=one(-1.0),
                       depth1=one(1.0), depth2=one(0.0), level1=one(0, np.int32), level2=one(0, np.int32)))
    return [(a, K4, default_params(cos_parallax_max=2.0), DEGENERATE, TRIANGULATE), (b, kb, default_params(), ZERO_DIST, UNPROJECT_1)]


def keyframe_scene(n, n_depth, c, seed, th_depth=3.5, ties=True, has_share=0.3):
    """n features of which n_depth have a depth > 0, c of them <= th_depth; ties in depth (broken by index) and features that already have a point"""
    rng = np.random.default_rng(seed)
    assert c <= n_depth <= n
    depth = np.zeros(n)
    near = np.round(rng.uniform(0.5, th_depth, c), 1 if ties else 9)
    far_ = np.round(rng.uniform(th_depth + 0.1, 30.0, n_depth - c), 1 if ties else 9)
    if c:
        near[0] = th_depth                      # exactly on the bound: close
    vals = np.concatenate([near, far_])
    idx = rng.permutation(n)[:n_depth]
    depth[idx] = vals
    rest = np.setdiff1d(np.arange(n), idx)
    depth[rest] = np.where(rng.random(len(rest)) < 0.5, 0.0, -1.0)
    px = np.stack([rng.uniform(0, WIDTH, n), rng.uniform(0, HEIGHT, n)], 1)
    has = (rng.random(n) < has_share).astype(np.uint8)
    T = np.concatenate([small_quat(rng, 0.3), rng.normal(size=3)])
    return T, px, depth, has


KEYFRAME_GRID = [(nd, c) for nd in (0, 1, 99, 100, 101, 500) for c in sorted({0, 50, 100, 101, nd}) if c <= nd]
