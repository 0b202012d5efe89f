"""The definition of the stereo odometry on resident slots (ygz_hip_stereo_odometry_slots, ygz_slam_amd/csrc/svo.hip) as a
composition: strack_ref.search (tests/strack_ref.c) and popt_ref.optimize (tests/popt_ref.c) joined by three formulas -- the un-projection of
the last frame's keypoints with a depth, the right column of the current frame's keypoints, and the edge list of the matches.  Nothing else is
computed here.  tests/test_svo_ref.py checks it on exact synthetic arrays, tests/test_gpu_svo.py holds the device call to it bit for bit.  Test
infrastructure: never imported by the package."""
import numpy as np

import popt_ref
import strack_ref

DEFAULTS = dict(baseline=0.1, th=7.0, th_dist=100, check_orientation=1, min_matches=20)
INT_OUTPUTS = strack_ref.INT_OUTPUTS
COUNTS = ("last_keypoints", "with_depth", "cur_keypoints", "matches", "searched", "overflowed", "removed_by_orientation", "retried")
IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])


def has_depth(depth, has_mp):
    """formula 0: a keypoint has a depth when its flag is set and the depth is above zero (a NaN is not)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(has_mp) != 0) & (np.asarray(depth, np.float64) > 0)


def unproject(px, depth, has, K):
    """formula 1: pw = (((u - cx) / fx) z, ((v - cy) / fy) z, z) for a point with a depth, 0 and the skip flag for one without"""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    z = np.where(has, np.asarray(depth, np.float64), 0.0)
    pw = np.stack([((px[:, 0] - K[2]) / K[0]) * z, ((px[:, 1] - K[3]) / K[1]) * z, z], axis=1)
    return np.where(has[:, None], pw, 0.0), (~has).astype(np.uint8)


def right_columns(px, depth, has, baseline, K):
    """formula 2: kp_ur = u - bf / depth with bf = fx baseline formed once, -1 without a depth (popt_ref.uright_from_depth)"""
    px = np.asarray(px, np.float64).reshape(-1, 2)
    return popt_ref.uright_from_depth(px[:, 0], np.where(has, np.asarray(depth, np.float64), 0.0), baseline, K[0])


def edges(match, pw, kp_px, kp_ur, kp_level):
    """formula 3: the matched points in point order: (point indices, X, obs = (kx, ky, kp_ur), level, kind 2 with a right column >= 0 else 1)"""
    idx = np.flatnonzero(np.asarray(match) >= 0)
    j = np.asarray(match)[idx]
    ur = np.asarray(kp_ur, np.float64)[j]
    obs = np.concatenate([np.asarray(kp_px, np.float64).reshape(-1, 2)[j], ur[:, None]], axis=1).reshape(-1, 3)
    return idx, np.asarray(pw, np.float64).reshape(-1, 3)[idx], obs, np.asarray(kp_level, np.int32)[j], np.where(ur >= 0, 2, 1).astype(np.uint8)


def pose_params(baseline, **fields):
    """ygz_hip_default_pose_opt_params with the call's baseline, then the given fields"""
    return popt_ref.defaults(**dict(dict(baseline=baseline), **fields))


def track_pair(last, cur, T_init=None, direction=None, K=popt_ref.DEFAULT_K, w=640, h=480, L=3, pose=None, **kw):
    """one pair.  last, cur: dicts of px [n, 2], level, angle (float32 degrees), desc [n, 32], depth, has_mp.  The outputs of the call for that
    pair, every per-point output by the last frame's keypoint (not padded)"""
    prm = dict(DEFAULTS, **kw)
    baseline = prm["baseline"]
    T0 = IDENTITY.copy() if T_init is None else np.array(T_init, np.float64).reshape(7)
    if direction is None:
        direction = strack_ref.direction(IDENTITY, T0, baseline)
    n_pt, n_kp = len(np.asarray(last["level"]).reshape(-1)), len(np.asarray(cur["level"]).reshape(-1))
    hl, hc = has_depth(last["depth"], last["has_mp"]), has_depth(cur["depth"], cur["has_mp"])
    pw, skip = unproject(last["px"], last["depth"], hl, K)
    ur = right_columns(cur["px"], cur["depth"], hc, baseline, K)
    s = dict(pw=pw, pt_desc=np.asarray(last["desc"], np.uint8).reshape(-1, 32), pt_level=np.asarray(last["level"], np.int32),
             pt_angle=np.asarray(last["angle"], np.float32).astype(np.float64))
    b = dict(T=T0, mode=strack_ref.FRAME, direction=int(direction), kp_px=np.asarray(cur["px"], np.float64).reshape(-1, 2),
             kp_level=np.asarray(cur["level"], np.int32), kp_desc=np.asarray(cur["desc"], np.uint8).reshape(-1, 32), kp_ur=ur,
             kp_angle=np.asarray(cur["angle"], np.float32).astype(np.float64), pt_skip=skip, set=0)
    search = lambda th: strack_ref.search([s], [dict(b, th=th)], K4=K, w=w, h=h, L=L, baseline=baseline, th_dist=prm["th_dist"],
                                          check_orientation=prm["check_orientation"])
    o, retried = search(prm["th"]), 0
    if o["counts"][0, 0] < prm["min_matches"]:
        o, retried = search(2.0 * prm["th"]), 1
    status = 1 if o["counts"][0, 0] < prm["min_matches"] else 0
    out = {k: o[k] for k in INT_OUTPUTS}
    out["proj"], out["rot"] = o["proj"], o["rot"][0]
    out["counts"] = np.array([n_pt, int(hl.sum()), n_kp] + [int(v) for v in o["counts"][0]] + [retried], np.int32)
    out["status"], out["retried"] = status, retried
    idx, X, obs, lvl, kind = edges(o["match"] if status == 0 else np.full(n_pt, -1), pw, b["kp_px"], ur, b["kp_level"])
    pp = pose if pose is not None else pose_params(baseline)
    pp.baseline = baseline
    r = popt_ref.optimize(popt_ref.Frame(X, obs, lvl, kind, T0), pp, K)
    out["T_rel"] = r["pose"]
    out["outlier"], out["chi2"] = np.zeros(n_pt, np.uint8), np.full(n_pt, -1.0)
    out["outlier"][idx], out["chi2"][idx] = r["outlier"], r["chi2"]
    out["inliers"], out["rounds_run"] = r["inliers"], r["rounds_run"]
    out["round_status"] = r["status"]
    for k in ("lm_iterations", "cost_initial", "cost_final", "lambda"):
        out[k] = r[k]
    out["edges"] = idx
    return out


def padded(pairs_out, cells):
    """the outputs of a call from those of its pairs: [n, cells], -1 (proj 0, outlier 0, chi2 -1.0) past a pair's last keypoint"""
    n = len(pairs_out)
    o = {k: np.full((n, cells), -1, np.int32) for k in INT_OUTPUTS}
    o.update(proj=np.zeros((n, cells, 3)), outlier=np.zeros((n, cells), np.uint8), chi2=np.full((n, cells), -1.0))
    for k in ("T_rel", "rot", "counts", "round_status", "lm_iterations", "cost_initial", "cost_final", "lambda"):
        o[k] = np.stack([q[k] for q in pairs_out])
    for k in ("status", "inliers", "rounds_run"):
        o[k] = np.array([q[k] for q in pairs_out], np.int32)
    for p, q in enumerate(pairs_out):
        m = len(q["match"])
        for k in INT_OUTPUTS + ("proj", "outlier", "chi2"):
            o[k][p, :m] = q[k]
    return o


def odometry(frames, last_slots, cur_slots, cells, T_init=None, direction=None, **kw):
    """the call: frames maps a slot to its arrays; the padded outputs of all pairs"""
    outs = []
    for p, (l, c) in enumerate(zip(last_slots, cur_slots)):
        outs.append(track_pair(frames[int(l)], frames[int(c)], None if T_init is None else np.asarray(T_init, np.float64).reshape(-1, 7)[p],
                               None if direction is None else int(np.asarray(direction).reshape(-1)[p]), **kw))
    return padded(outs, cells)


# ---- exact synthetic frames ---------------------------------------------------------------------------------------------------------------
def se3_apply(T, X):
    return np.asarray(X, np.float64) @ popt_ref.w_rotation(np.asarray(T, np.float64)).T + np.asarray(T, np.float64)[4:]


def se3_mul(a, b):
    """a o b: first b, then a"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    q = popt_ref.w_qmul(a[:4], b[:4])
    return np.concatenate([q / np.linalg.norm(q), popt_ref.w_rotation(a) @ b[4:] + a[4:]])


# 0.1 m forward and 0.21 degrees about an oblique axis, as a literal quaternion (its norm is 1 to the last bit): last camera -> current camera
TRUTH = np.array([0.001, -0.0015, 0.0005, 0.9999982499984688, 0.0, 0.0, -0.1])


def exact_scene(n=300, seed=7, truth=TRUTH, K=popt_ref.DEFAULT_K, w=640, h=480, baseline=0.1, z_range=(8.0, 20.0)):
    """(last, cur): n points in front of the last camera with exact depths; the current camera's keypoints are their exact projections at
    `truth` (last camera -> current camera), with exact depths there; point i and keypoint i share a random descriptor, level 0, angle 0"""
    rng = np.random.default_rng(seed)
    # keypoints on a jittered grid, far enough apart that no window of 7 pixels holds two of them
    cols = int(np.ceil(np.sqrt(n * w / h)))
    rows = int(np.ceil(n / cols))
    gx, gy = (w - 120.0) / cols, (h - 120.0) / rows
    cell = np.arange(n)
    px = np.stack([60 + (cell % cols + 0.5) * gx + rng.uniform(-2, 2, n), 60 + (cell // cols + 0.5) * gy + rng.uniform(-2, 2, n)], 1)
    z = rng.uniform(z_range[0], z_range[1], n)
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    zeros = np.zeros(n, np.int32)
    last = dict(px=px, level=zeros, angle=np.zeros(n, np.float32), desc=desc, depth=z, has_mp=np.ones(n, np.uint8))
    pw, _ = unproject(px, z, np.ones(n, bool), K)
    Pc = se3_apply(truth, pw)
    cpx = np.stack([K[0] * (Pc[:, 0] / Pc[:, 2]) + K[2], K[1] * (Pc[:, 1] / Pc[:, 2]) + K[3]], 1)
    assert (Pc[:, 2] > 0).all() and (cpx[:, 0] > 0).all() and (cpx[:, 0] < w).all() and (cpx[:, 1] > 0).all() and (cpx[:, 1] < h).all()
    cur = dict(px=cpx, level=zeros, angle=np.zeros(n, np.float32), desc=desc.copy(), depth=Pc[:, 2].copy(), has_mp=np.ones(n, np.uint8))
    return last, cur
