"""The definition of the stereo reference-keyframe tracking on resident slots (ygz_hip_stereo_ref_keyframe_slots, ygz_slam_amd/csrc/srk.hip,
DESIGN.md section 29) as a composition: the oracle's yo_bow_transform, yo_search_by_bow and yo_bow_orientation (oracle/bow.c) and
popt_ref.optimize (tests/popt_ref.c) joined by these formulas -- the masked node row of the keyframe, the right column of the frame's
keypoints, the claim of a frame keypoint by the smallest keyframe feature, the bin of a claimed match and its removal, the point every frame
keypoint ends with, the edge list in keypoint order, and prior = kp_point without the optimiser's outliers.  Nothing else is computed here.
tests/test_srk_ref.py checks it on exact synthetic arrays, tests/test_gpu_srk.py holds the device call to it bit for bit.  Test
infrastructure: never imported by the package."""
import numpy as np

import popt_ref
import slm_ref as sl
import svo_ref as sv

DEFAULTS = dict(baseline=0.1, th_low=50, knn_ratio=0.7, levelsup=4, check_orientation=1, min_matches=15, min_inliers=10)
MAX_FRAMES, MAX_KEYFRAMES, MAX_SETS = 1024, 256, 64
COUNTS = ("keyframe_keypoints", "with_point", "keypoints", "with_right_column", "search_matches", "lost_claim", "removed_by_orientation", "edges")
MATCHED, NO_MATCH, LOST_CLAIM, ORIENTATION = 0, 1, 2, 4
IDENTITY = sv.IDENTITY
has_depth, right_columns, pose_params, se3_apply, se3_mul = sv.has_depth, sv.right_columns, sv.pose_params, sv.se3_apply, sv.se3_mul
_ORACLE = []


def oracle():
    if not _ORACLE:
        from oracle.pyoracle import Oracle
        _ORACLE.append(Oracle())
    return _ORACLE[0]


def masked_nodes(node, kf_point):
    """formula 1: the keyframe's FeatureVector node where the keypoint carries a point, -1 where it does not"""
    return np.where(np.asarray(kf_point) >= 0, np.asarray(node, np.int32), -1).astype(np.int32)


def claim(match, n2):
    """formula 2 (the used[] rule): frame keypoint j goes to the smallest i with match[i] == j; (holder [n2] with -1 for a free keypoint, lost
    [n1])"""
    match = np.asarray(match, np.int32)
    holder = np.full(n2, -1, np.int32)
    lost = np.zeros(len(match), bool)
    for i, j in enumerate(match):
        if j < 0:
            continue
        if holder[j] < 0:
            holder[j] = i
        else:
            lost[i] = True
    return holder, lost


def c_round(x):
    """C's round: half away from zero (numpy's rounds half to even)"""
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def rotation_bins(angle1, angle2, match):
    """formula 3: the histogram bin of every match as yo_bow_orientation computes it (float rot, + 360 when negative, the float factor 1 / 30,
    C round, 30 -> 0), -1 outside the histogram and for an entry without a match"""
    match = np.asarray(match, np.int32)
    a1, a2 = np.asarray(angle1, np.float32).astype(np.float64), np.asarray(angle2, np.float32).astype(np.float64)
    out = np.full(len(match), -1, np.int32)
    i = np.flatnonzero(match >= 0)
    rot = (a1[i] - a2[match[i]]).astype(np.float32)
    rot = np.where(rot < 0, rot + np.float32(360), rot).astype(np.float32)
    b = c_round((rot * (np.float32(1.0) / np.float32(30))).astype(np.float32)).astype(np.int64)
    b[b == 30] = 0
    out[i] = np.where((b >= 0) & (b < 30), b, -1)
    return out


def orientation(angle1, angle2, match):
    """step 5: (hist [30], the three maxima, removed [n1]): the histogram and the maxima are the oracle's, a match in another bin is removed"""
    match = np.asarray(match, np.int32)
    a1, a2 = np.asarray(angle1, np.float32).astype(np.float64), np.asarray(angle2, np.float32).astype(np.float64)
    _, hist, ind = oracle().bow_orientation(a1, a2 if len(a2) else np.zeros(1), match)
    bins = rotation_bins(angle1, angle2, match)
    keep = (bins >= 0) & np.isin(bins, ind[ind >= 0])
    return hist.astype(np.int32), ind.astype(np.int32), (match >= 0) & ~keep


def keypoint_points(match, kf_point, n2):
    """formula 4: the set index behind every frame keypoint: kf_point of the keyframe feature that holds it, -1 without one"""
    kp_point = np.full(n2, -1, np.int32)
    i = np.flatnonzero(np.asarray(match) >= 0)
    kp_point[np.asarray(match)[i]] = np.asarray(kf_point, np.int32)[i]
    return kp_point


edges = sl.edges                                                        # formula 5: the keypoints with a point in KEYPOINT order


def prior_of(kp_point, outlier):
    """formula 6: what the frame hands to the local-map stage: kp_point with the optimiser's outliers dropped"""
    return np.where(np.asarray(outlier) != 0, -1, np.asarray(kp_point, np.int32)).astype(np.int32)


def nodes(vocab, desc, levelsup):
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    return oracle().bow_transform(vocab, desc, levelsup)[2].astype(np.int32) if len(desc) else np.zeros(0, np.int32)


def track_frame(kfr, fr, kf_point, s, T, vocab, K=popt_ref.DEFAULT_K, pose=None, **kw):
    """one frame.  kfr, fr: dicts of px [n, 2], level, angle (float32 degrees), desc [n, 32], depth, has_mp (a slot's arrays); kf_point [n1]
    (longer rows are cut); s: dict with pw.  The outputs of the call for that frame, the per-keypoint ones by keypoint, not padded"""
    prm = dict(DEFAULTS, **kw)
    baseline = prm["baseline"]
    T0 = np.array(T, np.float64).reshape(7)
    n1, n2 = len(np.asarray(kfr["level"]).reshape(-1)), len(np.asarray(fr["level"]).reshape(-1))
    kfp = np.asarray(kf_point, np.int32).reshape(-1)[:n1]
    pw = np.asarray(s.get("pw", np.zeros((0, 3))), np.float64).reshape(-1, 3)
    d1, d2 = np.asarray(kfr["desc"], np.uint8).reshape(-1, 32), np.asarray(fr["desc"], np.uint8).reshape(-1, 32)
    node1, node2 = masked_nodes(nodes(vocab, d1, prm["levelsup"]), kfp), nodes(vocab, d2, prm["levelsup"])
    ur = right_columns(fr["px"], fr["depth"], has_depth(fr["depth"], fr["has_mp"]), baseline, K)
    found, _ = oracle().search_by_bow(d1, node1, d2, node2, prm["th_low"], prm["knn_ratio"])
    found = found.astype(np.int32).copy()
    outcome = np.where(kfp >= 0, np.where(found >= 0, MATCHED, NO_MATCH), -1).astype(np.int32)
    _, lost = claim(found, n2)
    match = np.where(lost, -1, found).astype(np.int32)
    outcome[lost] = LOST_CLAIM
    hist, ind, removed = np.zeros(30, np.int32), np.full(3, -1, np.int32), np.zeros(n1, bool)
    if prm["check_orientation"]:
        hist, ind, removed = orientation(kfr["angle"], fr["angle"], match)
    match[removed] = -1
    outcome[removed] = ORIENTATION
    kp_point = keypoint_points(match, kfp, n2)
    kp_px, kp_level = np.asarray(fr["px"], np.float64).reshape(-1, 2), np.asarray(fr["level"], np.int32).reshape(-1)
    j, X, obs, lvl, kind = edges(kp_point, pw, kp_px, ur, kp_level)
    n_edges = len(j)
    status = 1 if n_edges < prm["min_matches"] else 0
    if status:                                                           # too few: the optimiser is given no edge
        j, X, obs, lvl, kind = j[:0], X[:0], obs[:0], lvl[:0], kind[:0]
    pp = pose if pose is not None else pose_params(baseline)
    pp.baseline = baseline
    r = popt_ref.optimize(popt_ref.Frame(X, obs, lvl, kind, T0), pp, K)
    if status == 0 and r["inliers"] < prm["min_inliers"]:
        status = 2
    out = dict(T_out=r["pose"], status=status, kp_point=kp_point, match12=match, outcome=outcome, rot=np.concatenate([hist, ind]).astype(np.int32))
    out["counts"] = np.array([n1, int((kfp >= 0).sum()), n2, int((ur >= 0).sum()), int((found >= 0).sum()), int(lost.sum()), int(removed.sum()),
                              n_edges], np.int32)
    out["outlier"], out["chi2"] = np.zeros(n2, np.uint8), np.full(n2, -1.0)
    out["outlier"][j], out["chi2"][j] = r["outlier"], r["chi2"]
    out["prior"] = prior_of(kp_point, out["outlier"])
    out["inliers"], out["rounds_run"], out["round_status"] = r["inliers"], r["rounds_run"], r["status"]
    for k in ("lm_iterations", "cost_initial", "cost_final", "lambda"):
        out[k] = r[k]
    out["edges"], out["kp_ur"], out["node1"], out["node2"], out["found"] = j, ur, node1, node2, found
    return out


PER_CELL = ("kp_point", "prior", "outlier", "chi2", "match12", "outcome")


def joined(frames_out, cells):
    """the outputs of a call from those of its frames: the per-keypoint ones [n, cells] with -1 (outlier 0, chi2 -1.0) past the last keypoint"""
    n = len(frames_out)
    o = {k: np.full((n, cells), -1, np.int32) for k in ("kp_point", "prior", "match12", "outcome")}
    o.update(outlier=np.zeros((n, cells), np.uint8), chi2=np.full((n, cells), -1.0))
    for k in ("T_out", "counts", "rot", "round_status", "lm_iterations", "cost_initial", "cost_final", "lambda"):
        o[k] = np.stack([q[k] for q in frames_out])
    for k in ("status", "inliers", "rounds_run"):
        o[k] = np.array([q[k] for q in frames_out], np.int32)
    for f, q in enumerate(frames_out):
        for k in PER_CELL:
            o[k][f, :len(q[k])] = q[k]
    return o


def ref_keyframe(frames, sets, kf_slot, kf_set, kf_point, slot, kf, T, vocab, cells, **kw):
    """the call: frames maps a slot to its arrays, sets is the list of point sets, kf_point [n_kf][cells]"""
    T = np.asarray(T, np.float64).reshape(-1, 7)
    kf_point = np.asarray(kf_point, np.int32).reshape(len(kf_slot), -1)
    outs = []
    for f, (sl_, k) in enumerate(zip(slot, kf)):
        outs.append(track_frame(frames[int(kf_slot[int(k)])], frames[int(sl_)], kf_point[int(k)], sets[int(kf_set[int(k)])], T[f], vocab, **kw))
    return joined(outs, cells)


# ---- the exact synthetic scene ------------------------------------------------------------------------------------------------------------
TRUTH = sv.TRUTH


def exact_scene(n=300, seed=3, truth=TRUTH, K=popt_ref.DEFAULT_K):
    """(keyframe, frame, set): svo_ref.exact_scene with the keyframe's camera as the world: n world points 8 .. 20 m in front of the keyframe,
    its keypoints and the frame's their exact projections with exact depths, the frame at `truth` (world -> camera); point i, keyframe
    keypoint i and frame keypoint i share a random descriptor; level 0, angle 0"""
    kfr, fr = sv.exact_scene(n, seed, truth, K)
    pw, _ = sv.unproject(kfr["px"], kfr["depth"], np.ones(n, bool), K)
    return kfr, fr, dict(pw=pw)
