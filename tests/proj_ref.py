"""ctypes loader of tests/proj_ref.c, the restatement of the projection-guided descriptor search (ygz_slam_amd/csrc/proj.hip) that
tests/test_proj_ref.py and tests/test_gpu_projection.py hold ygz_hip_search_by_projection against.  Test infrastructure: compiled with gcc into
a temporary directory the first time it is used, never imported by the package.  Also the seeded synthetic scenes of the tests."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOPK = 8
KEPT, SKIP, BEHIND, OUTSIDE, RANGE, ANGLE = range(6)
K4_DEFAULT = np.array([520.9, 521.0, 325.1, 249.7], np.float32).astype(np.float64)     # config/default.yaml:32-35 (float intrinsics)
DEFAULTS = dict(th=10.0, th_dist=50, claim=1)
_lib = None


class PrProblem(ctypes.Structure):
    """pr_problem of proj_ref.c (the layout of ygz_proj_problem, include/ygz_hip.h)"""
    _fields_ = [("kp_px", ctypes.POINTER(ctypes.c_double)), ("kp_level", ctypes.POINTER(ctypes.c_int32)),
                ("kp_desc", ctypes.POINTER(ctypes.c_uint8)), ("kp_taken", ctypes.POINTER(ctypes.c_uint8)), ("n_kp", ctypes.c_int),
                ("pw", ctypes.POINTER(ctypes.c_double)), ("pt_desc", ctypes.POINTER(ctypes.c_uint8)), ("pt_dmax", ctypes.POINTER(ctypes.c_double)),
                ("pt_normal", ctypes.POINTER(ctypes.c_double)), ("pt_skip", ctypes.POINTER(ctypes.c_uint8)), ("n_pt", ctypes.c_int),
                ("S", ctypes.c_double * 8)]


class PrParams(ctypes.Structure):
    _fields_ = [("th", ctypes.c_double), ("th_dist", ctypes.c_int), ("claim", ctypes.c_int)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="proj_ref_")
        so = os.path.join(d, "libproj_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "proj_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(**kw):
    p = PrParams()
    for k, v in dict(DEFAULTS, **kw).items():
        setattr(p, k, v)
    return p


def _problems(problems):
    arr = (PrProblem * len(problems))()
    keep = []

    def put(d, name, dtype, shape, ct):
        a = d.get(name)
        if a is None:
            return ctypes.POINTER(ct)()
        a = np.ascontiguousarray(a, dtype).reshape(shape)
        keep.append(a)
        return _p(a, ct)
    for q, d in enumerate(problems):
        b = arr[q]
        b.kp_px = put(d, "kp_px", np.float64, (-1, 2), ctypes.c_double)
        b.kp_level = put(d, "kp_level", np.int32, (-1,), ctypes.c_int32)
        b.kp_desc = put(d, "kp_desc", np.uint8, (-1, 32), ctypes.c_uint8)
        b.kp_taken = put(d, "kp_taken", np.uint8, (-1,), ctypes.c_uint8)
        b.pw = put(d, "pw", np.float64, (-1, 3), ctypes.c_double)
        b.pt_desc = put(d, "pt_desc", np.uint8, (-1, 32), ctypes.c_uint8)
        b.pt_dmax = put(d, "pt_dmax", np.float64, (-1,), ctypes.c_double)
        b.pt_normal = put(d, "pt_normal", np.float64, (-1, 3), ctypes.c_double)
        b.pt_skip = put(d, "pt_skip", np.uint8, (-1,), ctypes.c_uint8)
        b.n_kp, b.n_pt = len(d["kp_level"]), len(d["pt_dmax"])
        b.S = (ctypes.c_double * 8)(*[float(v) for v in d["S"]])
    return arr, keep


def candidates(problem, K4=K4_DEFAULT, w=640, h=480, L=3, **kw):
    """steps 1-8 of one problem: cand_idx, cand_dist [n][8], n_cand, pred_level, reason [n], uv [n][2]"""
    arr, keep = _problems([problem])
    n = arr[0].n_pt
    ci, cd = np.zeros((n, TOPK), np.int32), np.zeros((n, TOPK), np.int32)
    nc, pl, why, uv = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 2))
    K = np.ascontiguousarray(K4, np.float64)
    p = params(**kw)
    lib().pr_candidates(arr, _p(K, ctypes.c_double), w, h, L, ctypes.byref(p), _p(ci, ctypes.c_int32), _p(cd, ctypes.c_int32),
                        _p(nc, ctypes.c_int32), _p(pl, ctypes.c_int32), _p(why, ctypes.c_int32), _p(uv, ctypes.c_double))
    return dict(cand_idx=ci, cand_dist=cd, n_cand=nc, pred_level=pl, reason=why, uv=uv)


def search(problems, K4=K4_DEFAULT, w=640, h=480, L=3, **kw):
    """the fused call: match, dist, pred_level [N] concatenated over the problems, counts [P][2]"""
    arr, keep = _problems(problems)
    N = sum(arr[q].n_pt for q in range(len(problems)))
    match, dist, pl = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    counts = np.zeros((len(problems), 2), np.int32)
    K = np.ascontiguousarray(K4, np.float64)
    p = params(**kw)
    lib().pr_search(len(problems), arr, _p(K, ctypes.c_double), w, h, L, ctypes.byref(p), _p(match, ctypes.c_int32), _p(dist, ctypes.c_int32),
                    _p(pl, ctypes.c_int32), _p(counts, ctypes.c_int32))
    return dict(match=match, dist=dist, pred_level=pl, counts=counts)


# ---- seeded synthetic scenes ------------------------------------------------------------------------------------------------------------
def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_S(rng, s=1.0):
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    th = np.deg2rad(rng.uniform(2, 25))
    q = np.concatenate([np.sin(th / 2) * a, [np.cos(th / 2)]])
    return np.concatenate([q, rng.uniform(-0.4, 0.4, 3), [s]])


def flip_bits(rng, desc, k):
    d = np.unpackbits(desc.copy())
    d[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(d)


def scene(n_pt, n_kp, seed, s=1.0, normals=True, taken=False, skip=False, K4=K4_DEFAULT, w=640, h=480, L=3, stray=0.25):
    """n_kp keypoints of random pixels, levels and descriptors, and n_pt points: a fraction 1 - stray sits within a few pixels of a keypoint's
    ray at a depth whose ratio dmax / d predicts that keypoint's level or the one above, with the keypoint's descriptor and 0-70 flipped bits
    (several points may pick one keypoint: the claim has contention); the rest are anywhere (behind the camera, outside the image, out of
    range, facing away).  kp_taken / pt_skip mark a tenth each when asked for."""
    rng = np.random.default_rng(seed)
    S = random_S(rng, s)
    R, t = quat_to_R(S[:4]), S[4:7]
    kp_px = np.stack([rng.uniform(0, w, n_kp), rng.uniform(0, h, n_kp)], 1)
    kp_level = rng.integers(0, L, n_kp).astype(np.int32)
    kp_desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    Xc, dmax, desc, nrm = np.zeros((n_pt, 3)), np.zeros(n_pt), np.zeros((n_pt, 32), np.uint8), np.zeros((n_pt, 3))
    for i in range(n_pt):
        if rng.uniform() < stray:
            z = rng.uniform(-2, 8)
            px = np.array([rng.uniform(-60, w + 60), rng.uniform(-60, h + 60)])
            ratio = 2.0 ** rng.uniform(-1.0, L + 0.5)
            desc[i] = rng.integers(0, 256, 32)
            facing = rng.uniform() < 0.7
        else:
            j = int(rng.integers(0, n_kp))
            z = rng.uniform(1.5, 7)
            lv = int(kp_level[j]) + int(rng.integers(0, 2))                       # the keypoint's level or the one above
            px = kp_px[j] + rng.uniform(-1, 1, 2) * rng.choice([3.0, 9.0, 25.0])
            ratio = 2.0 ** min(lv, L - 1) * rng.uniform(0.55, 0.98)
            desc[i] = flip_bits(rng, kp_desc[j], int(rng.integers(0, 71)))
            facing = rng.uniform() < 0.9
        x = np.array([(px[0] - K4[2]) / K4[0] * z, (px[1] - K4[3]) / K4[1] * z, z])
        Xc[i] = x
        d = np.linalg.norm(x)
        dmax[i] = ratio * d
        view = -x / max(d, 1e-9)                                                  # from the point towards the camera, camera frame
        tilt = rng.normal(size=3) * (0.3 if facing else 2.0)
        nc = -(view + tilt) if facing else (view + tilt)                          # ORB-SLAM2's normal points from the camera to the point
        nrm[i] = R.T @ (nc / np.linalg.norm(nc)) * rng.uniform(0.7, 1.0)          # a mean of unit rays: not of unit length
    pw = ((Xc - t) @ R) / s
    out = dict(kp_px=kp_px, kp_level=kp_level, kp_desc=kp_desc, pw=pw, pt_desc=desc, pt_dmax=dmax, S=S)
    if normals:
        out["pt_normal"] = nrm
    if taken:
        out["kp_taken"] = (rng.uniform(size=n_kp) < 0.1).astype(np.uint8)
    if skip:
        out["pt_skip"] = (rng.uniform(size=n_pt) < 0.1).astype(np.uint8)
    return out
