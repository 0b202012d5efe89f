"""ctypes loader of tests/strack_ref.c, the restatement of the stereo tracking search (ygz_slam_amd/csrc/strack.hip) that
tests/test_strack_ref.py and tests/test_gpu_strack.py hold ygz_hip_stereo_track_search against.  Test infrastructure: compiled with gcc into a
temporary directory the first time it is used, never imported by the package.  Also the seeded scenes of the tests, and the Python
restatements of StereoTracker's host rules (motion direction, LocalKeyFrames, the visible / found bookkeeping) on a map of plain dicts."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import lfuse_ref as lf
import proj_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
FRAME, LOCAL = 0, 1
SEARCHED, SKIP, BEHIND, OUTSIDE, RANGE, ANGLE = range(6)
MATCHED, NO_CANDIDATE, DISTANCE, RATIO, ORIENTATION = range(5)
K4_DEFAULT = pr.K4_DEFAULT
DEFAULTS = dict(baseline=0.1, ratio=0.8, r_near=2.5, r_wide=4.0, cos_near=0.998, th_dist=100, check_orientation=1)
PARAM_FIELDS = ["baseline", "ratio", "r_near", "r_wide", "cos_near", "th_dist", "check_orientation"]
POINTS_FIELDS = ["pw", "pt_desc", "pt_level", "pt_angle", "pt_dmax", "pt_normal", "n_pt"]
PROBLEM_FIELDS = ["T", "th", "kp_px", "kp_level", "kp_desc", "kp_ur", "kp_angle", "kp_taken", "pt_skip", "n_kp", "set", "mode", "direction"]
MAX_PROBLEMS, MAX_SETS, MAX_PAIRS, TOPK = 64, 8, 262144, 8
INT_OUTPUTS = ("match", "dist", "level", "reason", "outcome", "n_cand", "n_gated")
_lib = None
_dp, _ip, _bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)


class Points(ctypes.Structure):
    """st_points of strack_ref.c (the layout of ygz_strack_points, include/ygz_hip.h)"""
    _fields_ = [("pw", _dp), ("pt_desc", _bp), ("pt_level", _ip), ("pt_angle", _dp), ("pt_dmax", _dp), ("pt_normal", _dp), ("n_pt", ctypes.c_int)]


class Problem(ctypes.Structure):
    """st_problem (ygz_strack_problem)"""
    _fields_ = [("T", ctypes.c_double * 7), ("th", ctypes.c_double), ("kp_px", _dp), ("kp_level", _ip), ("kp_desc", _bp), ("kp_ur", _dp),
                ("kp_angle", _dp), ("kp_taken", _bp), ("pt_skip", _bp), ("n_kp", ctypes.c_int), ("set", ctypes.c_int), ("mode", ctypes.c_int),
                ("direction", ctypes.c_int)]


class Params(ctypes.Structure):
    """st_params (ygz_strack_params)"""
    _fields_ = [("baseline", ctypes.c_double), ("ratio", ctypes.c_double), ("r_near", ctypes.c_double), ("r_wide", ctypes.c_double),
                ("cos_near", ctypes.c_double), ("th_dist", ctypes.c_int32), ("check_orientation", ctypes.c_int32)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="strack_ref_")
        so = os.path.join(d, "libstrack_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "strack_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        for f in ("st_points_size", "st_problem_size", "st_params_size", "st_offset"):
            getattr(_lib, f).restype = ctypes.c_size_t
    return _lib


def params(cls=Params, **kw):
    p = cls()
    for k, v in dict(DEFAULTS, **kw).items():
        setattr(p, k, v)
    return p


def default_params():
    p = Params()
    p.check_orientation = 9
    lib().st_default_params(ctypes.byref(p))
    return p


def set_size(d):
    return len(np.asarray(d["pt_desc"]).reshape(-1)) // 32 if d.get("pt_desc") is not None else 0


def c_arrays(sets, problems, points_cls=Points, problem_cls=Problem):
    """the two struct arrays of a call from lists of dicts, and the numpy arrays they point into (keep them alive).  A set: pw, pt_desc,
    pt_level, pt_angle, pt_dmax, pt_normal; a problem: T, th, mode, direction, kp_px, kp_level, kp_desc, kp_ur, kp_angle, kp_taken, pt_skip, set"""
    keep = []

    def put(d, name, dtype, ct):
        a = d.get(name)
        if a is None:
            return ctypes.POINTER(ct)()
        a = np.ascontiguousarray(a, dtype).reshape(-1)
        keep.append(a)
        return a.ctypes.data_as(ctypes.POINTER(ct))
    sa = (points_cls * max(len(sets), 1))()
    for s, d in enumerate(sets):
        sa[s].pw = put(d, "pw", np.float64, ctypes.c_double)
        sa[s].pt_desc = put(d, "pt_desc", np.uint8, ctypes.c_uint8)
        sa[s].pt_level = put(d, "pt_level", np.int32, ctypes.c_int32)
        sa[s].pt_angle = put(d, "pt_angle", np.float64, ctypes.c_double)
        sa[s].pt_dmax = put(d, "pt_dmax", np.float64, ctypes.c_double)
        sa[s].pt_normal = put(d, "pt_normal", np.float64, ctypes.c_double)
        sa[s].n_pt = d.get("force_n", set_size(d))
    pa = (problem_cls * max(len(problems), 1))()
    for q, d in enumerate(problems):
        T = np.asarray(d["T"], np.float64).reshape(7)
        for k in range(7):
            pa[q].T[k] = T[k]
        pa[q].th = d.get("th", 7.0)
        pa[q].kp_px = put(d, "kp_px", np.float64, ctypes.c_double)
        pa[q].kp_level = put(d, "kp_level", np.int32, ctypes.c_int32)
        pa[q].kp_desc = put(d, "kp_desc", np.uint8, ctypes.c_uint8)
        pa[q].kp_ur = put(d, "kp_ur", np.float64, ctypes.c_double)
        pa[q].kp_angle = put(d, "kp_angle", np.float64, ctypes.c_double)
        pa[q].kp_taken = put(d, "kp_taken", np.uint8, ctypes.c_uint8)
        pa[q].pt_skip = put(d, "pt_skip", np.uint8, ctypes.c_uint8)
        pa[q].n_kp = d.get("force_n_kp", len(np.asarray(d["kp_level"]).reshape(-1)) if d.get("kp_level") is not None else 1)
        pa[q].set = d.get("set", 0)
        pa[q].mode = d.get("mode", 0)
        pa[q].direction = d.get("direction", 0)
    return sa, pa, keep


def offsets(sets, problems):
    return np.concatenate([[0], np.cumsum([set_size(sets[p.get("set", 0)]) for p in problems])]).astype(np.int64)


def search(sets, problems, K4=K4_DEFAULT, w=640, h=480, L=3, **kw):
    """the call on the restatement: the outputs of ygz_hip_stereo_track_search, concatenated in problem order"""
    sa, pa, keep = c_arrays(sets, problems)
    N, Q = int(offsets(sets, problems)[-1]), len(problems)
    o = {k: np.full(max(N, 1), -7, np.int32) for k in INT_OUTPUTS}
    proj, cand = np.zeros((max(N, 1), 3)), np.full((max(N, 1), TOPK), -7, np.int32)
    counts, rot = np.zeros((Q, 4), np.int32), np.zeros((Q, 33), np.int32)
    K = np.ascontiguousarray(K4, np.float64)
    p = params(**kw)
    lib().st_search(len(sets), sa, Q, pa, K.ctypes.data_as(_dp), w, h, L, ctypes.byref(p), *[o[k].ctypes.data_as(_ip) for k in INT_OUTPUTS],
                    proj.ctypes.data_as(_dp), cand.ctypes.data_as(_ip), counts.ctypes.data_as(_ip), rot.ctypes.data_as(_ip))
    del keep
    o = {k: v[:N] for k, v in o.items()}
    o["proj"], o["cand"], o["counts"], o["rot"] = proj[:N], cand[:N], counts, rot
    return o


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------------
def hamming_matrix(a, b):
    """[len(a)][len(b)] Hamming distances of 32-byte descriptors"""
    A, B = np.unpackbits(np.asarray(a, np.uint8), axis=1).astype(np.int32), np.unpackbits(np.asarray(b, np.uint8), axis=1).astype(np.int32)
    return A.sum(1)[:, None] + B.sum(1)[None, :] - 2 * (A @ B.T)


def local_scene(n_pt, n_kp, seed, th=3.0, **kw):
    """lfuse_ref.scene as (sets, problems) of one LOCAL problem: right columns on about 60 % of the keypoints"""
    sc = lf.scene(n_pt, n_kp, seed, **kw)
    s, p = lf.split(sc)
    p.update(mode=LOCAL, th=th, direction=0)
    return [s], [p]


def frame_scene(n_pt, n_kp, seed, direction=0, th=7.0, L=3, angles=True, turn=20.0, **kw):
    """the same scene as one FRAME problem: a point takes the level of the keypoint whose descriptor it was derived from, that level or a
    neighbour; with angles, every keypoint a random angle and a point that keypoint's angle plus `turn` and up to 3 degrees (a sixth: any)"""
    sc = lf.scene(n_pt, n_kp, seed, L=L, **kw)
    rng = np.random.default_rng(seed + 104729)
    s, p = lf.split(sc)
    near = hamming_matrix(sc["pt_desc"], sc["kp_desc"]).argmin(1)
    s.pop("pt_dmax", None); s.pop("pt_normal", None)
    s["pt_level"] = np.clip(sc["kp_level"][near] + rng.choice([-1, 0, 0, 0, 1], n_pt), 0, L - 1).astype(np.int32)
    if angles:
        p["kp_angle"] = rng.uniform(0, 360, n_kp)
        any_ = rng.uniform(size=n_pt) < 1 / 6
        s["pt_angle"] = np.where(any_, rng.uniform(0, 360, n_pt), np.mod(p["kp_angle"][near] + turn + rng.uniform(-3, 3, n_pt), 360.0))
    p.update(mode=FRAME, th=th, direction=direction)
    return [s], [p]


def contention_scene(seed, mode, n_pt=96, n_kp=24, L=3):
    """several points want one keypoint: n_pt points on the rays of n_kp keypoints, a few bits apart"""
    rng = np.random.default_rng(seed)
    K4 = K4_DEFAULT
    kp_px = np.stack([rng.uniform(40, 600, n_kp), rng.uniform(40, 440, n_kp)], 1)
    kp_level = rng.integers(0, L, n_kp).astype(np.int32)
    kp_desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    j = rng.integers(0, n_kp, n_pt)
    z = rng.uniform(2, 6, n_pt)
    px = kp_px[j] + rng.uniform(-0.9, 0.9, (n_pt, 2))
    pw = np.stack([(px[:, 0] - K4[2]) / K4[0] * z, (px[:, 1] - K4[3]) / K4[1] * z, z], 1)
    d = np.linalg.norm(pw, axis=1)
    desc = np.stack([pr.flip_bits(rng, kp_desc[jj], int(rng.integers(0, 20))) for jj in j])
    s = dict(pw=pw, pt_desc=desc)
    p = dict(T=np.array([0, 0, 0, 1.0, 0, 0, 0]), kp_px=kp_px, kp_level=kp_level, kp_desc=kp_desc, set=0, mode=mode, direction=0,
             th=7.0 if mode == FRAME else 1.0)
    if mode == FRAME:
        s["pt_level"] = kp_level[j]
    else:
        s["pt_dmax"] = 2.0 ** kp_level[j] * 0.9 * d
        s["pt_normal"] = pw / d[:, None]
    return [s], [p]


def overflow_scene(seed, mode, n_pt=40, per=12, L=3):
    """every point has `per` keypoints of its level inside its window: n_cand > TOPK"""
    rng = np.random.default_rng(seed)
    K4 = K4_DEFAULT
    z = rng.uniform(2, 6, n_pt)
    px = np.stack([rng.uniform(40, 600, n_pt), rng.uniform(40, 440, n_pt)], 1)
    pw = np.stack([(px[:, 0] - K4[2]) / K4[0] * z, (px[:, 1] - K4[3]) / K4[1] * z, z], 1)
    d = np.linalg.norm(pw, axis=1)
    lv = rng.integers(0, L, n_pt).astype(np.int32)
    desc = rng.integers(0, 256, (n_pt, 32)).astype(np.uint8)
    kp_px = (px[:, None, :] + rng.uniform(-0.9, 0.9, (n_pt, per, 2))).reshape(-1, 2)
    kp_level = np.repeat(lv, per)
    kp_desc = np.stack([pr.flip_bits(rng, desc[i], int(rng.integers(0, 90))) for i in np.repeat(np.arange(n_pt), per)])
    s = dict(pw=pw, pt_desc=desc)
    p = dict(T=np.array([0, 0, 0, 1.0, 0, 0, 0]), kp_px=kp_px, kp_level=kp_level, kp_desc=kp_desc, set=0, mode=mode, direction=0,
             th=7.0 if mode == FRAME else 1.0)
    if mode == FRAME:
        s["pt_level"] = lv
    else:
        s["pt_dmax"] = 2.0 ** lv * 0.9 * d
        s["pt_normal"] = pw / d[:, None]
    return [s], [p]


def ratio_scene(seed, n_pt=60, L=3):
    """LOCAL: every point has two keypoints of its level in the window, 10 and 11 .. 30 bits away: the ratio rule fires where 10 > 0.8 d2"""
    rng = np.random.default_rng(seed)
    K4 = K4_DEFAULT
    z = rng.uniform(2, 6, n_pt)
    px = np.stack([rng.uniform(40, 600, n_pt), rng.uniform(40, 440, n_pt)], 1)
    pw = np.stack([(px[:, 0] - K4[2]) / K4[0] * z, (px[:, 1] - K4[3]) / K4[1] * z, z], 1)
    d = np.linalg.norm(pw, axis=1)
    lv = rng.integers(0, L, n_pt).astype(np.int32)
    desc = rng.integers(0, 256, (n_pt, 32)).astype(np.uint8)
    kp_px = (px[:, None, :] + rng.uniform(-0.9, 0.9, (n_pt, 2, 2))).reshape(-1, 2)
    second = rng.integers(11, 31, n_pt)
    kp_desc = np.stack([pr.flip_bits(rng, desc[i], 10 if k == 0 else int(second[i])) for i in range(n_pt) for k in range(2)])
    s = dict(pw=pw, pt_desc=desc, pt_dmax=2.0 ** lv * 0.9 * d, pt_normal=pw / d[:, None])
    p = dict(T=np.array([0, 0, 0, 1.0, 0, 0, 0]), kp_px=kp_px, kp_level=np.repeat(lv, 2), kp_desc=kp_desc, set=0, mode=LOCAL, direction=0, th=1.0)
    return [s], [p]


def decoy_scene(n_pt, seed, with_columns=True, th=7.0, K4=K4_DEFAULT, w=640, h=480, baseline=0.1):
    """FRAME, levels 0 .. 2, identity pose: point i has its true keypoint (index n_pt + i, within 2 px, its descriptor with 5 flipped bits, the
    right column of the point's depth) and ONE decoy (index i, within 2 px, the point's exact descriptor, a right column off by r + 1 .. r + 30
    px).  The points sit on a grid whose cells are wider than two windows, so no point sees another's keypoints.  with_columns False:
    kp_ur = -1 throughout"""
    rng = np.random.default_rng(seed)
    bf = K4[0] * baseline
    lv = rng.integers(0, 3, n_pt).astype(np.int32)
    r = th * 2.0 ** lv
    cols = 10
    gx, gy = 62.0, 62.0
    cell = np.arange(n_pt)
    frames = cell // (cols * 7)                                        # more points than one image holds: the grid repeats at another depth
    cell = cell % (cols * 7)
    px = np.stack([31 + (cell % cols) * gx + rng.uniform(-1, 1, n_pt), 31 + (cell // cols) * gy + rng.uniform(-1, 1, n_pt)], 1)
    z = 2.0 + 0.05 * frames + rng.uniform(0, 0.01, n_pt)
    pw = np.stack([(px[:, 0] - K4[2]) / K4[0] * z, (px[:, 1] - K4[3]) / K4[1] * z, z], 1)
    desc = rng.integers(0, 256, (n_pt, 32)).astype(np.uint8)
    true_px = px + rng.uniform(-2, 2, (n_pt, 2))
    decoy_px = px + rng.uniform(-2, 2, (n_pt, 2))
    true_desc = np.stack([pr.flip_bits(rng, desc[i], 5) for i in range(n_pt)])
    ur = px[:, 0] - bf / z
    true_ur = ur + rng.uniform(-1, 1, n_pt)
    decoy_ur = ur + (r + rng.uniform(1, 30, n_pt))
    s = dict(pw=pw, pt_desc=desc, pt_level=lv)
    p = dict(T=np.array([0, 0, 0, 1.0, 0, 0, 0]), kp_px=np.concatenate([decoy_px, true_px]), kp_level=np.concatenate([lv, lv]),
             kp_desc=np.concatenate([desc, true_desc]), set=0, mode=FRAME, direction=0, th=th)
    p["kp_ur"] = np.concatenate([decoy_ur, true_ur]) if with_columns else np.full(2 * n_pt, -1.0)
    return [s], [p]


def mixed_scene(n_problems, n_pt, n_kp, seed, L=3):
    """n_problems problems over two point sets (one FRAME, one LOCAL), modes and directions mixed"""
    fs, fp = frame_scene(n_pt, n_kp, seed, L=L)
    ls, lp = local_scene(n_pt, n_kp, seed + 1, L=L)
    sets, problems = [fs[0], ls[0]], []
    rng = np.random.default_rng(seed + 2)
    for q in range(n_problems):
        base = dict(fp[0] if q % 2 == 0 else lp[0])
        base["set"] = q % 2
        base["direction"] = int(rng.integers(-1, 2)) if q % 2 == 0 else 0
        if q >= 2:
            T = np.asarray(base["T"], np.float64).copy()
            T[4:7] += rng.uniform(-0.02, 0.02, 3)
            base["T"] = T
        problems.append(base)
    return sets, problems


# ---- the host rules of StereoTracker on plain data ----------------------------------------------------------------------------------------
def direction(T_last, T_cur, baseline, has_columns=True):
    """t_lc = R_l (-R_c^T t_c) + t_l: +1 when t_lc.z > baseline, -1 when -t_lc.z > baseline, else 0; 0 for a tracker without right columns"""
    if not has_columns:
        return 0
    Rl, Rc = pr.quat_to_R(np.asarray(T_last[:4], np.float64)), pr.quat_to_R(np.asarray(T_cur[:4], np.float64))
    t_lc = Rl @ (-(Rc.T @ np.asarray(T_cur[4:7], np.float64))) + np.asarray(T_last[4:7], np.float64)
    return 1 if t_lc[2] > baseline else (-1 if -t_lc[2] > baseline else 0)


def local_keyframes(points_on_frame, points, keyframes, neighbours=10, max_keyframes=80):
    """points_on_frame: the ids of the current frame's map points (None: no point), points: {id: dict(bad, obs {kf id: feature index})},
    keyframes: {kf id: dict(bad, cov [kf ids, best first])}.  Returns (the list, the reference keyframe or None)"""
    votes = {}
    for pid in points_on_frame:
        if pid is None or points[pid]["bad"]:
            continue
        for k in points[pid]["obs"]:
            votes[k] = votes.get(k, 0) + 1
    out = [k for k in sorted(votes) if not keyframes[k]["bad"]]
    ref = None
    for k in sorted(votes):
        if ref is None or votes[k] > votes[ref]:
            ref = k
    for k in list(out):
        if len(out) >= max_keyframes:
            break
        for c in keyframes[k]["cov"][:neighbours]:
            if not keyframes[c]["bad"] and c not in out:
                out.append(c)
                break
    return out, ref


def track_local_bookkeeping(on_frame, local_points, reason, match, inliers):
    """the counters TrackLocalMap moves: on_frame the good points already on the frame (visible + 1 each), local_points the searched list with
    the device's reason (0: visible + 1, in view) and match (>= 0: the feature takes the point); inliers: the points the optimiser kept (found
    + 1).  Returns {id: (visible, found, in_view)} of the increments"""
    out = {}
    for pid in on_frame:
        v, f, _ = out.get(pid, (0, 0, False))
        out[pid] = (v + 1, f, False)
    for pid, why in zip(local_points, reason):
        v, f, _ = out.get(pid, (0, 0, False))
        out[pid] = (v + (1 if why == 0 else 0), f, why == 0)
    for pid in inliers:
        v, f, iv = out.get(pid, (0, 0, False))
        out[pid] = (v, f + 1, iv)
    return out
