"""The definition of the stereo relocalisation on resident slots (ygz_hip_stereo_relocalize_slots, ygz_slam_amd/csrc/srl.hip, DESIGN.md
section 32) as a composition: steps 1 to 6 of the reference-keyframe call (the formulas of tests/srk_ref.py around the oracle's
yo_bow_transform, yo_search_by_bow and yo_bow_orientation), pr_ransac of tests/pnp_ref.c on the associations in keypoint order, and
popt_ref.optimize (tests/popt_ref.c) on the PnP inliers from the PnP pose, joined by these formulas -- the skip of a problem with too few
associations, the edge list of the PnP inliers, prior = kp_point of the PnP inliers that are no optimiser outliers, the status, and the first
problem of a frame with status 0.  Nothing else is computed here.  tests/test_srl_ref.py checks it on exact synthetic arrays,
tests/test_gpu_srl.py holds the device call to it bit for bit.  Test infrastructure: never imported by the package."""
import numpy as np

import pnp_ref
import popt_ref
import srk_ref as sk

DEFAULTS = dict(baseline=0.1, th_low=50, knn_ratio=0.75, levelsup=4, check_orientation=1, min_matches=15, min_final_inliers=50)
PNP_DEFAULTS = dict(max_iter=300, chi2=5.991, min_inliers=10)
MAX_FRAMES, MAX_PROBLEMS, MAX_KEYFRAMES, MAX_SETS, MAX_HYPOTHESIS_SETS = 256, 256, 256, 64, 76800
COUNTS = sk.COUNTS + ("pnp_inliers", "final_inliers")
RELOCALISED, TOO_FEW_MATCHES, PNP_FAILED, TOO_FEW_INLIERS = 0, 1, 2, 3
IDENTITY = sk.IDENTITY
PNP_INTS = ("success", "n_inliers", "best_sample", "best_solution", "n_hypotheses")


def associate(kfr, fr, kf_point, s, vocab, K, prm):
    """step 1: steps 1 to 6 of srk_ref.track_frame.  Dict of the per-keypoint outputs and the associations j (frame keypoints, ascending),
    X, obs (kx, ky, uR), level, kind"""
    n1, n2 = len(np.asarray(kfr["level"]).reshape(-1)), len(np.asarray(fr["level"]).reshape(-1))
    kfp = np.asarray(kf_point, np.int32).reshape(-1)[:n1]
    pw = np.asarray(s.get("pw", np.zeros((0, 3))), np.float64).reshape(-1, 3)
    d1, d2 = np.asarray(kfr["desc"], np.uint8).reshape(-1, 32), np.asarray(fr["desc"], np.uint8).reshape(-1, 32)
    node1, node2 = sk.masked_nodes(sk.nodes(vocab, d1, prm["levelsup"]), kfp), sk.nodes(vocab, d2, prm["levelsup"])
    ur = sk.right_columns(fr["px"], fr["depth"], sk.has_depth(fr["depth"], fr["has_mp"]), prm["baseline"], K)
    found, _ = sk.oracle().search_by_bow(d1, node1, d2, node2, prm["th_low"], prm["knn_ratio"])
    found = found.astype(np.int32).copy()
    outcome = np.where(kfp >= 0, np.where(found >= 0, sk.MATCHED, sk.NO_MATCH), -1).astype(np.int32)
    _, lost = sk.claim(found, n2)
    match = np.where(lost, -1, found).astype(np.int32)
    outcome[lost] = sk.LOST_CLAIM
    hist, ind, removed = np.zeros(30, np.int32), np.full(3, -1, np.int32), np.zeros(n1, bool)
    if prm["check_orientation"]:
        hist, ind, removed = sk.orientation(kfr["angle"], fr["angle"], match)
    match[removed] = -1
    outcome[removed] = sk.ORIENTATION
    kp_point = sk.keypoint_points(match, kfp, n2)
    kp_px, kp_level = np.asarray(fr["px"], np.float64).reshape(-1, 2), np.asarray(fr["level"], np.int32).reshape(-1)
    j, X, obs, lvl, kind = sk.edges(kp_point, pw, kp_px, ur, kp_level)
    counts = [n1, int((kfp >= 0).sum()), n2, int((ur >= 0).sum()), int((found >= 0).sum()), int(lost.sum()), int(removed.sum()), len(j)]
    return dict(kp_point=kp_point, match12=match, outcome=outcome, rot=np.concatenate([hist, ind]).astype(np.int32), counts=counts, j=j, X=X,
                obs=obs, level=lvl, kind=kind, n2=n2, kp_ur=ur)


def no_hypothesis():
    """what k_pnp_select writes for a problem none of whose hypotheses has an inlier, with n_hypotheses = 0"""
    return dict(R=np.eye(3).reshape(9), t=np.zeros(3), T_cw=IDENTITY.copy(), success=0, n_inliers=0, best_sample=-1, best_solution=-1,
                n_hypotheses=0)


def problem(kfr, fr, kf_point, s, vocab, K=popt_ref.DEFAULT_K, pose=None, pnp=None, **kw):
    """one problem: a frame against one candidate keyframe.  The outputs of the call for that problem, the per-keypoint ones not padded"""
    prm, pn = dict(DEFAULTS, **kw), dict(PNP_DEFAULTS, **(pnp or {}))
    a = associate(kfr, fr, kf_point, s, vocab, K, prm)
    n, n2, it = len(a["j"]), a["n2"], int(pn["max_iter"])
    pp = pose if pose is not None else sk.pose_params(prm["baseline"])
    pp.baseline = prm["baseline"]
    mask, sets = np.zeros(n, bool), np.zeros((it, 3), np.int32)
    if n < prm["min_matches"]:                                           # step 2: neither PnP nor optimisation
        status, res = TOO_FEW_MATCHES, no_hypothesis()
    else:                                                                # step 3: pr_ransac on the associations in keypoint order
        r = pnp_ref.ransac(a["X"], a["obs"][:, :2], np.array(K, np.float64), **pn)
        res, mask, sets = r["result"], r["inliers"], r["sets"]
        assert np.array_equal(sets, pnp_ref.sample_sets(n, it))
        status = RELOCALISED if res["success"] else PNP_FAILED
    T_pnp = np.array(res["T_cw"], np.float64)
    e = np.flatnonzero(mask) if status == RELOCALISED else np.zeros(0, np.int64)     # step 4: the PnP inliers, in keypoint order
    o = popt_ref.optimize(popt_ref.Frame(a["X"][e], a["obs"][e], a["level"][e], a["kind"][e], T_pnp), pp, K)
    if status == RELOCALISED and o["inliers"] < prm["min_final_inliers"]:
        status = TOO_FEW_INLIERS
    out = dict(status=status, T_pnp=T_pnp, T_opt=o["pose"], pnp=res, sets=sets)
    for k in ("kp_point", "match12", "outcome", "rot"):
        out[k] = a[k]
    out["counts"] = np.array(a["counts"] + [int(res["n_inliers"]), int(o["inliers"])], np.int32)
    out["pnp_inlier"], out["outlier"], out["chi2"] = np.zeros(n2, np.uint8), np.zeros(n2, np.uint8), np.full(n2, -1.0)
    out["pnp_inlier"][a["j"][mask]] = 1
    out["outlier"][a["j"][e]], out["chi2"][a["j"][e]] = o["outlier"], o["chi2"]
    out["prior"] = np.where((out["pnp_inlier"] != 0) & (out["outlier"] == 0), a["kp_point"], -1).astype(np.int32)
    out["inliers"], out["rounds_run"], out["round_status"] = o["inliers"], o["rounds_run"], o["status"]
    for k in ("lm_iterations", "cost_initial", "cost_final", "lambda"):
        out[k] = o[k]
    out["assoc"], out["edges"], out["kp_ur"] = a["j"], a["j"][e], a["kp_ur"]
    return out


PER_CELL = ("kp_point", "prior", "pnp_inlier", "outlier", "chi2", "match12", "outcome")


def joined(outs, cand_off, cells):
    """the outputs of a call from those of its problems: the per-keypoint ones [P, cells] with -1 (flags 0, chi2 -1.0) past the last keypoint,
    best and T_out per frame (step 5)"""
    n = len(outs)
    o = {k: np.full((n, cells), -1, np.int32) for k in ("kp_point", "prior", "match12", "outcome")}
    o.update(outlier=np.zeros((n, cells), np.uint8), pnp_inlier=np.zeros((n, cells), np.uint8), chi2=np.full((n, cells), -1.0))
    for k in ("T_pnp", "T_opt", "counts", "rot", "round_status", "lm_iterations", "cost_initial", "cost_final", "lambda", "sets"):
        o[k] = np.stack([q[k] for q in outs])
    for k in ("status", "inliers", "rounds_run"):
        o[k] = np.array([q[k] for q in outs], np.int32)
    for k in ("R", "t", "T_cw"):
        o["pnp_" + k] = np.stack([np.asarray(q["pnp"][k], np.float64).reshape(-1) for q in outs])
    for k in PNP_INTS:
        o["pnp_" + k] = np.array([q["pnp"][k] for q in outs], np.int32)
    for i, q in enumerate(outs):
        for k in PER_CELL:
            o[k][i, :len(q[k])] = q[k]
    F = len(cand_off) - 1
    o["best"], o["T_out"] = np.full(F, -1, np.int32), np.tile(IDENTITY, (F, 1))
    for f in range(F):
        ok = [q for q in range(int(cand_off[f]), int(cand_off[f + 1])) if outs[q]["status"] == RELOCALISED]
        if ok:
            o["best"][f], o["T_out"][f] = ok[0], outs[ok[0]]["T_opt"]
    return o


def offsets(candidates):
    """(cand_off, cand_kf) of the ragged list of candidate lists"""
    off = np.concatenate([[0], np.cumsum([len(c) for c in candidates])]).astype(np.int32)
    kf = np.array([k for c in candidates for k in c], np.int32)
    return off, kf


def relocalize(frames, sets, kf_slot, kf_set, kf_point, slot, candidates, vocab, cells, **kw):
    """the call: frames maps a slot to its arrays, sets is the list of point sets, kf_point [n_kf][cells], candidates[f] the ordered keyframe
    list of frame f"""
    kf_point = np.asarray(kf_point, np.int32).reshape(len(kf_slot), -1)
    off, ckf = offsets(candidates)
    outs = []
    for f, sl_ in enumerate(slot):
        for k in ckf[off[f]:off[f + 1]]:
            outs.append(problem(frames[int(kf_slot[int(k)])], frames[int(sl_)], kf_point[int(k)], sets[int(kf_set[int(k)])], vocab, **kw))
    return joined(outs, off, cells)
