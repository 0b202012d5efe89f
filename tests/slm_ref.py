"""The definition of the stereo local-map tracking on resident slots (ygz_hip_stereo_local_map_slots, ygz_slam_amd/csrc/slm.hip, DESIGN.md
section 28) as a composition: strack_ref.search in mode LOCAL (tests/strack_ref.c) and popt_ref.optimize (tests/popt_ref.c) joined by four
formulas -- the right column of the frame's keypoints, the taken / skip flags of the prior, the point each keypoint ends with, and the edge
list in keypoint order.  Nothing else is computed here.  tests/test_slm_ref.py checks it on exact synthetic arrays, tests/test_gpu_slm.py holds
the device call to it bit for bit.  Test infrastructure: never imported by the package."""
import numpy as np

import popt_ref
import strack_ref
import svo_ref as sv

DEFAULTS = dict(baseline=0.1, th=1.0, ratio=0.8, r_near=2.5, r_wide=4.0, cos_near=0.998, th_dist=100, min_edges=3)
MAX_FRAMES, MAX_SETS, MAX_PAIRS = 1024, 64, 4194304
INT_OUTPUTS = strack_ref.INT_OUTPUTS
COUNTS = ("keypoints", "with_right_column", "prior_edges", "points", "searched", "overflowed", "new_matches", "edges")
IDENTITY = sv.IDENTITY
has_depth, right_columns, pose_params, se3_apply, se3_mul = sv.has_depth, sv.right_columns, sv.pose_params, sv.se3_apply, sv.se3_mul


def prior_flags(prior, n_kp, n_pt):
    """formula 2: kp_taken[j] = (prior[j] >= 0); pt_skip[i] = 1 for every i the prior names.  prior None: all free"""
    pr = np.full(n_kp, -1, np.int32) if prior is None else np.asarray(prior, np.int32).reshape(-1)[:n_kp].copy()
    taken = (pr >= 0).astype(np.uint8)
    skip = np.zeros(n_pt, np.uint8)
    skip[pr[pr >= 0]] = 1
    return pr, taken, skip


def keypoint_points(pr, match):
    """formula 3: the point keypoint j ends with: prior[j] when that is >= 0, otherwise the point that claimed j, otherwise -1"""
    kp_point = pr.copy()
    idx = np.flatnonzero(np.asarray(match) >= 0)
    assert (kp_point[np.asarray(match)[idx]] == -1).all()              # a claimed keypoint was free
    kp_point[np.asarray(match)[idx]] = idx
    return kp_point


def edges(kp_point, pw, kp_px, kp_ur, kp_level):
    """formula 4: the keypoints with a point in KEYPOINT order: (keypoint indices, X = pw of the point, obs = (kx, ky, kp_ur), level, kind 2
    with a right column >= 0 else 1)"""
    j = np.flatnonzero(np.asarray(kp_point) >= 0)
    ur = np.asarray(kp_ur, np.float64)[j]
    obs = np.concatenate([np.asarray(kp_px, np.float64).reshape(-1, 2)[j], ur[:, None]], axis=1).reshape(-1, 3)
    X = np.asarray(pw, np.float64).reshape(-1, 3)[np.asarray(kp_point)[j]].reshape(-1, 3)
    return j, X, obs, np.asarray(kp_level, np.int32)[j], np.where(ur >= 0, 2, 1).astype(np.uint8)


def track_frame(fr, s, T, prior=None, K=popt_ref.DEFAULT_K, w=640, h=480, L=3, pose=None, **kw):
    """one frame.  fr: dict of px [n, 2], level, desc [n, 32], depth, has_mp (a slot's arrays); s: dict of pw, pt_desc, pt_dmax, pt_normal.
    The outputs of the call for that frame: the per-keypoint ones by keypoint, the per-point ones by point, neither padded"""
    prm = dict(DEFAULTS, **kw)
    baseline = prm["baseline"]
    T0 = np.array(T, np.float64).reshape(7)
    n_kp, n_pt = len(np.asarray(fr["level"]).reshape(-1)), strack_ref.set_size(s)
    ur = right_columns(fr["px"], fr["depth"], has_depth(fr["depth"], fr["has_mp"]), baseline, K)
    pr, taken, skip = prior_flags(prior, n_kp, n_pt)
    kp_px, kp_level = np.asarray(fr["px"], np.float64).reshape(-1, 2), np.asarray(fr["level"], np.int32).reshape(-1)
    b = dict(T=T0, th=prm["th"], mode=strack_ref.LOCAL, direction=0, kp_px=kp_px, kp_level=kp_level,
             kp_desc=np.asarray(fr["desc"], np.uint8).reshape(-1, 32), kp_ur=ur, kp_taken=taken, pt_skip=skip if n_pt else None, set=0)
    o = strack_ref.search([s], [b], K4=K, w=w, h=h, L=L, baseline=baseline, ratio=prm["ratio"], r_near=prm["r_near"], r_wide=prm["r_wide"],
                          cos_near=prm["cos_near"], th_dist=prm["th_dist"], check_orientation=0)
    out = {k: o[k] for k in INT_OUTPUTS}
    out["proj"] = o["proj"]
    kp_point = keypoint_points(pr, o["match"])
    j, X, obs, lvl, kind = edges(kp_point, s.get("pw", np.zeros((0, 3))), kp_px, ur, kp_level)
    n_edges = len(j)
    status = 1 if n_edges < prm["min_edges"] else 0
    if status:                                                           # too few: the optimiser is given no edge
        j, X, obs, lvl, kind = j[:0], X[:0], obs[:0], lvl[:0], kind[:0]
    pp = pose if pose is not None else pose_params(baseline)
    pp.baseline = baseline
    r = popt_ref.optimize(popt_ref.Frame(X, obs, lvl, kind, T0), pp, K)
    out["T_out"], out["status"], out["kp_point"] = r["pose"], status, kp_point
    out["counts"] = np.array([n_kp, int((ur >= 0).sum()), int((pr >= 0).sum()), n_pt, int(o["counts"][0, 1]), int(o["counts"][0, 2]),
                              int(o["counts"][0, 0]), n_edges], np.int32)
    out["outlier"], out["chi2"] = np.zeros(n_kp, np.uint8), np.full(n_kp, -1.0)
    out["outlier"][j], out["chi2"][j] = r["outlier"], r["chi2"]
    out["inliers"], out["rounds_run"], out["round_status"] = r["inliers"], r["rounds_run"], r["status"]
    for k in ("lm_iterations", "cost_initial", "cost_final", "lambda"):
        out[k] = r[k]
    out["edges"], out["kp_ur"] = j, ur
    return out


PER_KEYPOINT = ("kp_point", "outlier", "chi2")


def joined(frames_out, cells):
    """the outputs of a call from those of its frames: the per-keypoint ones [n, cells] with -1 (outlier 0, chi2 -1.0) past a frame's last
    keypoint, the per-point ones concatenated in frame order"""
    n = len(frames_out)
    o = dict(kp_point=np.full((n, cells), -1, np.int32), outlier=np.zeros((n, cells), np.uint8), chi2=np.full((n, cells), -1.0))
    for k in ("T_out", "counts", "round_status", "lm_iterations", "cost_initial", "cost_final", "lambda"):
        o[k] = np.stack([q[k] for q in frames_out])
    for k in ("status", "inliers", "rounds_run"):
        o[k] = np.array([q[k] for q in frames_out], np.int32)
    for f, q in enumerate(frames_out):
        m = len(q["kp_point"])
        for k in PER_KEYPOINT:
            o[k][f, :m] = q[k]
    for k in INT_OUTPUTS:
        o[k] = np.concatenate([q[k] for q in frames_out]).astype(np.int32)
    o["proj"] = np.concatenate([q["proj"].reshape(-1, 3) for q in frames_out]).reshape(-1, 3)
    o["offsets"] = np.concatenate([[0], np.cumsum([len(q["match"]) for q in frames_out])]).astype(np.int64)
    return o


def local_map(frames, sets, slot, set_, T, prior=None, cells=None, **kw):
    """the call: frames maps a slot to its arrays, sets is the list of point sets; prior None or a list with None / an array per frame"""
    outs = []
    T = np.asarray(T, np.float64).reshape(-1, 7)
    for f, (sl, st) in enumerate(zip(slot, set_)):
        outs.append(track_frame(frames[int(sl)], sets[int(st)], T[f], None if prior is None else prior[f], **kw))
    return joined(outs, cells)


# ---- exact synthetic scenes ---------------------------------------------------------------------------------------------------------------
# world -> camera: 0.2 degrees about an oblique axis as a literal quaternion (its norm is 1 to the last bit) and a small translation
TRUTH = np.array([0.001, -0.0015, 0.0005, 0.9999982499984688, 0.02, -0.01, 0.05])


def exact_scene(n=300, seed=7, truth=TRUTH, K=popt_ref.DEFAULT_K, w=640, h=480, z_range=(8.0, 20.0), L=3):
    """(frame, set): n keypoints on a jittered grid with exact depths, level 0; the world points are their exact un-projections carried back
    through `truth` (world -> camera), so the keypoints are the points' projections at `truth` to rounding; point i and keypoint i share a
    random descriptor; dmax makes level 0 the predicted level, the normal is the viewing direction"""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(n * w / h)))
    rows = int(np.ceil(n / cols))
    gx, gy = (w - 120.0) / cols, (h - 120.0) / rows
    cell = np.arange(n)
    px = np.stack([60 + (cell % cols + 0.5) * gx + rng.uniform(-2, 2, n), 60 + (cell // cols + 0.5) * gy + rng.uniform(-2, 2, n)], 1)
    z = rng.uniform(z_range[0], z_range[1], n)
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    Pc, _ = sv.unproject(px, z, np.ones(n, bool), K)
    R = popt_ref.w_rotation(np.asarray(truth, np.float64))
    pw = (Pc - np.asarray(truth, np.float64)[4:]) @ R                    # R^T (Pc - t)
    d = np.linalg.norm(Pc, axis=1)
    fr = dict(px=px, level=np.zeros(n, np.int32), desc=desc, depth=z, has_mp=np.ones(n, np.uint8))
    s = dict(pw=pw, pt_desc=desc.copy(), pt_dmax=0.9 * d, pt_normal=(Pc / d[:, None]) @ R)
    return fr, s
