"""ctypes loader of tests/lfuse_ref.c, the restatement of the local-map fusion search (ygz_slam_amd/csrc/lfuse.hip) that
tests/test_lfuse_ref.py and tests/test_gpu_lfuse.py hold ygz_hip_local_fuse_search against.  Test infrastructure: compiled with gcc into a
temporary directory the first time it is used, never imported by the package.  Also the seeded scenes of the tests, and the Python
restatement of StereoMapper::SearchInNeighbors' walk and of MapPointCulling's rule on a map of plain dicts."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import proj_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
SEARCHED, SKIP, BEHIND, OUTSIDE, RANGE, ANGLE = range(6)
K4_DEFAULT = pr.K4_DEFAULT
DEFAULTS = dict(th=3.0, baseline=0.1, chi2_mono=5.99, chi2_stereo=7.8, th_dist=50, pad=0)
PARAM_FIELDS = ["th", "baseline", "chi2_mono", "chi2_stereo", "th_dist", "pad"]
MAX_PROBLEMS, MAX_SETS, MAX_PAIRS = 64, 8, 1048576
_lib = None
_dp, _ip, _bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)


class Points(ctypes.Structure):
    """lf_points of lfuse_ref.c (the layout of ygz_lfuse_points, include/ygz_hip.h)"""
    _fields_ = [("pw", _dp), ("pt_desc", _bp), ("pt_dmax", _dp), ("pt_normal", _dp), ("n_pt", ctypes.c_int)]


class Problem(ctypes.Structure):
    """lf_problem (ygz_lfuse_problem)"""
    _fields_ = [("T", ctypes.c_double * 7), ("kp_px", _dp), ("kp_level", _ip), ("kp_desc", _bp), ("kp_ur", _dp), ("kp_taken", _bp), ("pt_skip", _bp),
                ("n_kp", ctypes.c_int), ("set", ctypes.c_int)]


class Params(ctypes.Structure):
    """lf_params (ygz_lfuse_params)"""
    _fields_ = [("th", ctypes.c_double), ("baseline", ctypes.c_double), ("chi2_mono", ctypes.c_double), ("chi2_stereo", ctypes.c_double),
                ("th_dist", ctypes.c_int32), ("pad", ctypes.c_int32)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="lfuse_ref_")
        so = os.path.join(d, "liblfuse_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "lfuse_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        for f in ("lf_points_size", "lf_problem_size", "lf_params_size", "lf_offset"):
            getattr(_lib, f).restype = ctypes.c_size_t
    return _lib


def params(cls=Params, **kw):
    p = cls()
    for k, v in dict(DEFAULTS, **kw).items():
        setattr(p, k, v)
    return p


def default_params():
    p = Params()
    p.pad = 9
    lib().lf_default_params(ctypes.byref(p))
    return p


def c_arrays(sets, problems, points_cls=Points, problem_cls=Problem):
    """the two struct arrays of a call from lists of dicts, and the numpy arrays they point into (keep them alive).  A set: pw, pt_desc,
    pt_dmax, pt_normal (optional); a problem: T, kp_px, kp_level, kp_desc, kp_ur, kp_taken, pt_skip (the last three optional), set"""
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
        sa[s].pt_dmax = put(d, "pt_dmax", np.float64, ctypes.c_double)
        sa[s].pt_normal = put(d, "pt_normal", np.float64, ctypes.c_double)
        sa[s].n_pt = d.get("force_n", len(np.asarray(d["pt_dmax"]).reshape(-1)) if d.get("pt_dmax") is not None else 0)
    pa = (problem_cls * max(len(problems), 1))()
    for q, d in enumerate(problems):
        T = np.asarray(d["T"], np.float64).reshape(7)
        for k in range(7):
            pa[q].T[k] = T[k]
        pa[q].kp_px = put(d, "kp_px", np.float64, ctypes.c_double)
        pa[q].kp_level = put(d, "kp_level", np.int32, ctypes.c_int32)
        pa[q].kp_desc = put(d, "kp_desc", np.uint8, ctypes.c_uint8)
        pa[q].kp_ur = put(d, "kp_ur", np.float64, ctypes.c_double)
        pa[q].kp_taken = put(d, "kp_taken", np.uint8, ctypes.c_uint8)
        pa[q].pt_skip = put(d, "pt_skip", np.uint8, ctypes.c_uint8)
        pa[q].n_kp = d.get("force_n_kp", len(np.asarray(d["kp_level"]).reshape(-1)) if d.get("kp_level") is not None else 1)
        pa[q].set = d.get("set", 0)
    return sa, pa, keep


def n_pairs(sets, problems):
    return sum(len(np.asarray(sets[p.get("set", 0)]["pt_dmax"]).reshape(-1)) for p in problems)


def offsets(sets, problems):
    return np.concatenate([[0], np.cumsum([len(np.asarray(sets[p.get("set", 0)]["pt_dmax"]).reshape(-1)) for p in problems])]).astype(np.int64)


def search(sets, problems, K4=K4_DEFAULT, w=640, h=480, L=3, **kw):
    """the call on the restatement: match, dist, pred_level, reason, n_gated [N] concatenated in problem order, counts [P][2]"""
    sa, pa, keep = c_arrays(sets, problems)
    N = n_pairs(sets, problems)
    o = {k: np.full(max(N, 1), -7, np.int32) for k in ("match", "dist", "pred_level", "reason", "n_gated")}
    counts = np.zeros((len(problems), 2), np.int32)
    K = np.ascontiguousarray(K4, np.float64)
    p = params(**kw)
    lib().lf_search(len(sets), sa, len(problems), pa, K.ctypes.data_as(_dp), w, h, L, ctypes.byref(p), *[o[k].ctypes.data_as(_ip) for k in
                    ("match", "dist", "pred_level", "reason", "n_gated")], counts.ctypes.data_as(_ip))
    del keep
    o = {k: v[:N] for k, v in o.items()}
    o["counts"] = counts
    return o


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------------
def camera_points(T, pw):
    R = pr.quat_to_R(np.asarray(T[:4], np.float64))
    return np.asarray(pw) @ R.T + np.asarray(T[4:7], np.float64)


def split(sc, set_index=0):
    """a proj_ref-style scene dict as (point set, problem)"""
    s = {k: sc[k] for k in ("pw", "pt_desc", "pt_dmax", "pt_normal") if k in sc}
    p = {k: sc[k] for k in ("kp_px", "kp_level", "kp_desc", "kp_ur", "kp_taken", "pt_skip") if k in sc}
    p["T"] = np.asarray(sc["S"][:7], np.float64)
    p["set"] = set_index
    return s, p


def scene(n_pt, n_kp, seed, stereo=0.6, baseline=0.1, K4=K4_DEFAULT, **kw):
    """proj_ref.scene with a right column on a fraction `stereo` of the keypoints: a keypoint that has a point projecting within 30 px takes the
    column of the nearest such point, u - bf / z, half of them with up to 1.5 px 2^level of noise and a tenth with up to 12 px (a wrong
    depth); every other keypoint a disparity of a depth of 1.5 .. 7 m.  A third of the base scene's points sit within 3 px of their keypoint:
    inside the window of th = 3."""
    sc = pr.scene(n_pt, n_kp, seed, K4=K4, **kw)
    rng = np.random.default_rng(seed + 7919)
    bf = K4[0] * baseline
    Xc = camera_points(sc["S"], sc["pw"])
    z = np.where(Xc[:, 2] > 0.05, Xc[:, 2], 1e9)
    uv = np.stack([K4[0] * Xc[:, 0] / z + K4[2], K4[1] * Xc[:, 1] / z + K4[3]], 1)
    ur_pt = uv[:, 0] - bf / z
    d2 = ((sc["kp_px"][:, None, :] - uv[None, :, :]) ** 2).sum(2)
    near = d2.argmin(1)
    has = d2[np.arange(n_kp), near] < 900.0
    kur = np.where(has, sc["kp_px"][:, 0] - (uv[near, 0] - ur_pt[near]), sc["kp_px"][:, 0] - bf / rng.uniform(1.5, 7, n_kp))
    kind = rng.uniform(size=n_kp)
    noise = np.where(kind < 0.5, rng.uniform(-1.5, 1.5, n_kp) * 2.0 ** sc["kp_level"], 0.0) + np.where(kind > 0.9, rng.uniform(-12, 12, n_kp), 0.0)
    kur = kur + noise
    mono = (rng.uniform(size=n_kp) >= stereo) | (kur < 0)
    sc["kp_ur"] = np.where(mono, -1.0, kur)
    return sc


def target(points, n_kp, seed, K4=K4_DEFAULT, w=640, h=480, L=3, stereo=0.6, baseline=0.1, taken=False, skip=False, T=None):
    """a target keyframe looking at an existing point set: a pose near `T` (default: a random one in front of the points), keypoints at the
    projections of randomly chosen points with 0 .. 4 px 2^level of offset, the predicted level or the one below, the point's descriptor with
    0 .. 60 flipped bits, a right column from the point's depth (with noise, a tenth from a wrong depth) on a fraction `stereo`"""
    rng = np.random.default_rng(seed)
    pw = np.asarray(points["pw"], np.float64).reshape(-1, 3)
    n_pt = len(pw)
    if T is None:
        T = pr.random_S(rng)[:7]
    T = np.asarray(T, np.float64).copy()
    bf = K4[0] * baseline
    kp_px, kp_level, kp_ur = np.zeros((n_kp, 2)), np.zeros(n_kp, np.int32), np.full(n_kp, -1.0)
    kp_desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    if n_pt:
        Xc = camera_points(T, pw)
        dmax = np.asarray(points["pt_dmax"], np.float64).reshape(-1)
    for j in range(n_kp):
        i = int(rng.integers(0, n_pt)) if n_pt else -1
        if i < 0 or Xc[i, 2] <= 0.1 or rng.uniform() < 0.15:
            kp_px[j] = [rng.uniform(0, w), rng.uniform(0, h)]
            kp_level[j] = rng.integers(0, L)
            if rng.uniform() < stereo:
                kp_ur[j] = max(kp_px[j, 0] - bf / rng.uniform(1.5, 7), -1.0)
            continue
        x, y, z = Xc[i]
        d = np.sqrt(x * x + y * y + z * z)
        pred = int(np.clip(np.ceil(np.log2(max(dmax[i] / d, 1e-9))), 0, L - 1))
        lv = max(pred - int(rng.integers(0, 2)), 0)
        off = rng.uniform(-1, 1, 2) * rng.choice([1.0, 2.5, 4.0]) * 2.0 ** lv
        u, v = K4[0] * x / z + K4[2], K4[1] * y / z + K4[3]
        kp_px[j] = [u + off[0], v + off[1]]
        kp_level[j] = lv
        kp_desc[j] = pr.flip_bits(rng, np.asarray(points["pt_desc"], np.uint8).reshape(-1, 32)[i], int(rng.integers(0, 61)))
        if rng.uniform() < stereo:
            r = rng.uniform()
            kur = kp_px[j, 0] - bf / z + (rng.uniform(-1.5, 1.5) * 2.0 ** lv if r < 0.5 else 0.0) + (rng.uniform(-12, 12) if r > 0.9 else 0.0)
            kp_ur[j] = kur if kur >= 0 else -1.0
    out = dict(T=T, kp_px=kp_px, kp_level=kp_level, kp_desc=kp_desc, kp_ur=kp_ur, set=0)
    if taken:
        out["kp_taken"] = (rng.uniform(size=n_kp) < 0.1).astype(np.uint8)
    if skip:
        out["pt_skip"] = (rng.uniform(size=n_pt) < 0.1).astype(np.uint8)
    return out


def point_set(n_pt, seed, normals=True, K4=K4_DEFAULT, w=640, h=480, L=3):
    """n_pt world points in front of the identity camera (a tenth anywhere), with dmax for a level 0 .. L-1, descriptors and normals"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.5, 7, n_pt)
    px = np.stack([rng.uniform(-40, w + 40, n_pt), rng.uniform(-40, h + 40, n_pt)], 1)
    stray = rng.uniform(size=n_pt) < 0.1
    z = np.where(stray, rng.uniform(-2, 8, n_pt), z)
    pw = np.stack([(px[:, 0] - K4[2]) / K4[0] * z, (px[:, 1] - K4[3]) / K4[1] * z, z], 1)
    d = np.maximum(np.linalg.norm(pw, axis=1), 1e-6)
    ratio = 2.0 ** rng.integers(0, L, n_pt) * rng.uniform(0.55, 0.98, n_pt) * np.where(stray, 2.0 ** rng.uniform(-2, 3, n_pt), 1.0)
    out = dict(pw=pw, pt_desc=rng.integers(0, 256, (n_pt, 32)).astype(np.uint8), pt_dmax=ratio * d)
    if normals:
        view = pw / d[:, None]
        tilt = rng.normal(size=(n_pt, 3)) * np.where(rng.uniform(size=n_pt) < 0.9, 0.3, 2.0)[:, None]
        n = view + tilt
        out["pt_normal"] = n / np.linalg.norm(n, axis=1)[:, None] * rng.uniform(0.7, 1.0, n_pt)[:, None]
    return out


def near_identity(rng):
    """a pose a few degrees and a few decimetres from the identity"""
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    th = np.deg2rad(rng.uniform(0.5, 6))
    return np.concatenate([np.sin(th / 2) * a, [np.cos(th / 2)], rng.uniform(-0.3, 0.3, 3)])


def shared_scene(n_pt, n_kp, n_problems, seed, **kw):
    """one point set and n_problems targets that all read it"""
    s = point_set(n_pt, seed, normals=kw.pop("normals", True))
    rng = np.random.default_rng(seed + 1)
    return [s], [target(s, n_kp, seed + 10 + q, T=near_identity(rng), **kw) for q in range(n_problems)]


def decoy_scene(n_pt, seed, with_columns=True, K4=K4_DEFAULT, w=640, h=480, L=3, baseline=0.1):
    """every point has ONE keypoint: within 2 px of its projection (a disc), of its predicted level, with its descriptor -- but the keypoint was
    measured at another depth: its right column differs from the point's by 3 .. 30 px.  Identity pose.  with_columns False: kp_ur = -1"""
    rng = np.random.default_rng(seed)
    bf = K4[0] * baseline
    z = rng.uniform(1.5, 7, n_pt)
    px = np.stack([rng.uniform(20, w - 20, n_pt), rng.uniform(20, h - 20, n_pt)], 1)
    pw = np.stack([(px[:, 0] - K4[2]) / K4[0] * z, (px[:, 1] - K4[3]) / K4[1] * z, z], 1)
    d = np.linalg.norm(pw, axis=1)
    lv = rng.integers(0, L, n_pt).astype(np.int32)
    dmax = 2.0 ** lv * rng.uniform(0.85, 0.98, n_pt) * d
    desc = rng.integers(0, 256, (n_pt, 32)).astype(np.uint8)
    ang, rad = rng.uniform(0, 2 * np.pi, n_pt), 2.0 * np.sqrt(rng.uniform(0, 1, n_pt))
    kp_px = px + np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    gap = rng.uniform(3, 30, n_pt) * rng.choice([-1.0, 1.0], n_pt)
    kur = kp_px[:, 0] - bf / z + gap
    kur = np.where(kur < 0, kp_px[:, 0] - bf / z + np.abs(gap), kur)
    s = dict(pw=pw, pt_desc=desc, pt_dmax=dmax)
    p = dict(T=np.array([0, 0, 0, 1.0, 0, 0, 0]), kp_px=kp_px, kp_level=lv, kp_desc=desc.copy(), set=0)
    if with_columns:
        p["kp_ur"] = kur
    else:
        p["kp_ur"] = np.full(n_pt, -1.0)
    return [s], [p]


# ---- the walk and the culling rule on a map of dicts ---------------------------------------------------------------------------------------
ADDED, REPLACED_INTO_POINT, REPLACED_INTO_FEATURE, CONFLICT = range(4)


def make_map(points, features, stereo):
    """points: {id: dict(bad, obs {kf id: feature index}, cnt_found, cnt_visible, first_seen)}; features: {kf id: [point id or -1]};
    stereo: {kf id: [bool]} (the feature has a right column).  Deep-copied"""
    return dict(points={i: dict(p, obs=dict(p["obs"])) for i, p in points.items()}, features={k: list(v) for k, v in features.items()},
                stereo={k: list(v) for k, v in stereo.items()})


def n_obs(m, pid):
    """ORB-SLAM2's Observations(): a stereo side counts 2, a mono side 1"""
    return sum(2 if m["stereo"][k][f] else 1 for k, f in m["points"][pid]["obs"].items())


def replace_map_point(m, src, dst):
    """LoopClosing::ReplaceMapPoint on the dict map"""
    if src == dst:
        return
    a, b = m["points"][src], m["points"][dst]
    for k in sorted(a["obs"]):
        f = a["obs"][k]
        if k not in b["obs"]:
            m["features"][k][f] = dst
            b["obs"][k] = f
        else:
            m["features"][k][f] = -1
    b["cnt_found"] += a["cnt_found"]
    b["cnt_visible"] += a["cnt_visible"]
    a["bad"] = True
    a["obs"] = {}


def walk(m, hits, touched=None):
    """hits: (target keyframe id, point id, feature index) in walk order.  Edits m; returns the actions (kind, target, point, feature, survivor)"""
    actions, into = [], {}
    touched = touched if touched is not None else set()
    for k, i, f in hits:
        P = i
        while P in into:
            P = into[P]
        pt = m["points"][P]
        if pt["bad"] or k in pt["obs"]:
            actions.append((CONFLICT, k, i, f, P))
            continue
        q = m["features"][k][f]
        if q < 0 or m["points"][q]["bad"]:
            if q >= 0:                                          # a bad point first loses the feature from its observations
                m["points"][q]["obs"] = {kk: ff for kk, ff in m["points"][q]["obs"].items() if not (kk == k and ff == f)}
            pt["obs"][k] = f
            m["features"][k][f] = P
            touched.add(k)
            actions.append((ADDED, k, i, f, P))
        elif q == P:
            continue
        elif n_obs(m, q) > n_obs(m, P):
            touched.update(m["points"][P]["obs"].keys())
            replace_map_point(m, P, q)
            into[P] = q
            actions.append((REPLACED_INTO_FEATURE, k, i, f, q))
        else:
            touched.update(m["points"][q]["obs"].keys())
            replace_map_point(m, q, P)
            into[q] = P
            actions.append((REPLACED_INTO_POINT, k, i, f, P))
    return actions


def cull(m, recent, c, min_obs=3, found_ratio=0.25):
    """MapPointCulling's rule: returns (the list afterwards, the ids set bad in order)"""
    keep, dead = [], []
    for pid in recent:
        p = m["points"][pid]
        kill = False
        if p["bad"]:
            continue
        if p["cnt_visible"] > 0 and np.float32(p["cnt_found"]) / np.float32(p["cnt_visible"]) < np.float32(found_ratio):
            kill = True
        elif c >= p["first_seen"] + 2 and n_obs(m, pid) <= min_obs:
            kill = True
        elif c >= p["first_seen"] + 3:
            continue
        if kill:
            for k, f in p["obs"].items():
                m["features"][k][f] = -1
            p["obs"] = {}
            p["bad"] = True
            dead.append(pid)
        else:
            keep.append(pid)
    return keep, dead
