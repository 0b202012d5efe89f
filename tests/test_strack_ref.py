"""The restatement of the stereo tracking search (tests/strack_ref.c) against a numpy witness written another way: the
rotation as a matrix product, the candidates by brute force over all keypoints, the predicted level as ceil(log2(dmax / d)), the claim as
ORB-SLAM2's literal sequential loop with a running best and second best, the three maxima by a stable sort.  Every output EQUAL for every point
that the witness does not mark as within 1e-9 relative of a threshold; the seeds are chosen so that no point is marked.  Also: LOCAL with the
gate open and the factors 1 is proj_ref.search with the claim; the orientation rule is the oracle's yo_bow_orientation; what the right column
buys on a scene of decoys; the Python restatements of StereoTracker's host rules on hand-made maps."""
import numpy as np
import pytest

import proj_ref as pr
import strack_ref as st

K4 = st.K4_DEFAULT
W, H = 640, 480
EPS = 1e-9
INT_NAMES = st.INT_OUTPUTS


def close(a, b):
    return np.abs(a - b) <= EPS * np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)


def witness_problem(s, p, L, prm):
    n = st.set_size(s)
    m = len(np.asarray(p["kp_level"]).reshape(-1))
    pw = np.asarray(s["pw"], np.float64).reshape(-1, 3)
    T = np.asarray(p["T"], np.float64)
    R = pr.quat_to_R(T[:4])
    Xc = pw @ R.T + T[4:7]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    mode, th, direction = p.get("mode", 0), p["th"], p.get("direction", 0)
    skip = np.asarray(p["pt_skip"]).astype(bool) if p.get("pt_skip") is not None else np.zeros(n, bool)
    bf = K4[0] * prm["baseline"]
    reason = np.full(n, -1)
    marked = np.zeros(n, bool)
    reason[skip] = st.SKIP
    live = reason < 0
    marked |= live & (np.abs(z) <= EPS)
    reason[live & ~(z > 0)] = st.BEHIND
    live = reason < 0
    zs = np.where(live, z, 1.0)
    u, v = K4[0] * x / zs + K4[2], K4[1] * y / zs + K4[3]
    marked |= live & (close(u, 0) | close(u, W) | close(v, 0) | close(v, H))
    reason[live & ~((u >= 0) & (u < W) & (v >= 0) & (v < H))] = st.OUTSIDE
    live = reason < 0
    ur = u - bf / zs
    level, lo, hi, r = np.full(n, -1), np.zeros(n, int), np.full(n, -1), np.zeros(n)
    if mode == st.FRAME:
        lvl = np.asarray(s["pt_level"]).astype(int)
        level = np.where(live, lvl, -1)
        r = th * 2.0 ** lvl
        lo, hi = {0: (lvl - 1, lvl + 1), 1: (lvl, np.full(n, L - 1)), -1: (np.zeros(n, int), lvl)}[direction]
    else:
        d = np.linalg.norm(Xc, axis=1)
        dmax = np.asarray(s["pt_dmax"], np.float64)
        dmin = dmax / 2.0 ** (L - 1)
        marked |= live & (close(d, 0.8 * dmin) | close(d, 1.2 * dmax))
        reason[live & ((d < 0.8 * dmin) | (d > 1.2 * dmax))] = st.RANGE
        live = reason < 0
        c = np.einsum("ij,ij->i", Xc, np.asarray(s["pt_normal"], np.float64).reshape(-1, 3) @ R.T)
        marked |= live & close(c, 0.5 * d)
        reason[live & (c < 0.5 * d)] = st.ANGLE
        live = reason < 0
        lg = np.log2(np.where(live, dmax / np.maximum(d, 1e-300), 1.0))
        marked |= live & (np.abs(lg - np.round(lg)) <= EPS)
        pred = np.clip(np.ceil(lg), 0, L - 1).astype(int)
        marked |= live & close(c, prm["cos_near"] * d)
        f = np.where(c > prm["cos_near"] * d, prm["r_near"], prm["r_wide"])
        level = np.where(live, pred, -1)
        r = th * f * 2.0 ** pred
        lo, hi = pred - 1, pred
    reason[live] = st.SEARCHED
    kp = np.asarray(p["kp_px"], np.float64).reshape(-1, 2)
    kl = np.asarray(p["kp_level"]).astype(int).reshape(-1)
    kur = np.asarray(p["kp_ur"], np.float64).reshape(-1) if p.get("kp_ur") is not None else np.full(m, -1.0)
    taken0 = np.asarray(p["kp_taken"]).astype(bool).reshape(-1) if p.get("kp_taken") is not None else np.zeros(m, bool)
    ham = st.hamming_matrix(np.asarray(s["pt_desc"], np.uint8).reshape(-1, 32), np.asarray(p["kp_desc"], np.uint8).reshape(-1, 32))
    dx, dy = np.abs(kp[None, :, 0] - u[:, None]), np.abs(kp[None, :, 1] - v[:, None])
    lv_ok = (kl[None, :] >= lo[:, None]) & (kl[None, :] <= hi[:, None]) & ~taken0[None, :] & live[:, None]
    marked |= (lv_ok & (close(dx, r[:, None]) | close(dy, r[:, None]))).any(1)
    window = lv_ok & (dx < r[:, None]) & (dy < r[:, None])
    er = np.abs(ur[:, None] - kur[None, :])
    stereo = kur[None, :] >= 0
    marked |= (window & stereo & close(er, r[:, None])).any(1)
    gated = window & stereo & (er > r[:, None])
    surv = window & ~gated
    n_cand, n_gated = surv.sum(1), gated.sum(1)
    cand = np.full((n, st.TOPK), -1)
    lists = []
    for i in range(n):
        js = np.nonzero(surv[i])[0]
        js = js[np.lexsort((js, ham[i, js]))][:st.TOPK]
        cand[i, :len(js)] = js
        lists.append(js)
    # ORB-SLAM2's loop: a running best and second best over the keypoints that nobody has yet, in index order
    taken = taken0.copy()
    match, dist, outcome = np.full(n, -1), np.full(n, -1), np.full(n, -1)
    for i in range(n):
        if reason[i] != st.SEARCHED:
            continue
        best, best2, bj, lev, lev2 = 257, 257, -1, -1, -1
        for j in sorted(lists[i]):
            if taken[j]:
                continue
            dd = ham[i, j]
            if dd < best:
                best2, lev2 = best, lev
                best, lev, bj = dd, kl[j], j
            elif dd < best2:
                best2, lev2 = dd, kl[j]
        if bj < 0:
            outcome[i] = st.NO_CANDIDATE
        elif best > prm["th_dist"]:
            outcome[i] = st.DISTANCE
        elif mode == st.LOCAL and best2 < 257 and lev == lev2 and best > prm["ratio"] * best2:
            outcome[i] = st.RATIO
        else:
            outcome[i], match[i], dist[i] = st.MATCHED, bj, best
            taken[bj] = True
    hist, ind, removed = np.zeros(30, int), [-1, -1, -1], 0
    if mode == st.FRAME and s.get("pt_angle") is not None and prm["check_orientation"]:
        mi = np.nonzero(match >= 0)[0]
        rot = (np.asarray(s["pt_angle"], np.float64)[mi] - np.asarray(p["kp_angle"], np.float64)[match[mi]]).astype(np.float32)
        rot = np.where(rot < 0, rot + np.float32(360), rot).astype(np.float32)
        b = np.floor((rot * (np.float32(1.0) / np.float32(30))).astype(np.float32).astype(np.float64) + 0.5).astype(int)
        b[b == 30] = 0
        ok = (b >= 0) & (b < 30)
        hist = np.bincount(b[ok], minlength=30)
        order = [k for k in sorted(range(30), key=lambda k: -hist[k]) if hist[k] > 0][:3]
        top = [hist[k] for k in order]
        if len(order) >= 2 and np.float32(top[1]) < np.float32(0.1) * np.float32(top[0]):
            order = order[:1]
        elif len(order) >= 3 and np.float32(top[2]) < np.float32(0.1) * np.float32(top[0]):
            order = order[:2]
        ind = (order + [-1, -1, -1])[:3]
        for k, i in enumerate(mi):
            if not ok[k] or b[k] not in order:
                match[i], dist[i], outcome[i] = -1, -1, st.ORIENTATION
                removed += 1
    proj = np.where((reason == st.SEARCHED)[:, None], np.stack([u, v, ur], 1), 0.0)
    srch = reason == st.SEARCHED
    counts = [int((match >= 0).sum()), int(srch.sum()), int((n_cand > st.TOPK).sum()), removed]
    return dict(match=match, dist=dist, level=level, reason=reason, outcome=outcome, n_cand=np.where(srch, n_cand, 0), n_gated=np.where(srch, n_gated, 0),
                proj=proj, cand=cand, counts=counts, rot=list(hist) + ind, marked=marked)


def witness(sets, problems, L=3, **kw):
    prm = dict(st.DEFAULTS, **kw)
    parts = [witness_problem(sets[p.get("set", 0)], p, L, prm) for p in problems]
    out = {k: np.concatenate([q[k] for q in parts]) for k in INT_NAMES + ("proj", "cand", "marked")}
    out["counts"], out["rot"] = np.array([q["counts"] for q in parts]), np.array([q["rot"] for q in parts])
    return out


def held(sets, problems, L=3, **kw):
    """the restatement equals the witness; no point is marked.  Returns the restatement's outputs"""
    got, want = st.search(sets, problems, K4, W, H, L, **kw), witness(sets, problems, L, **kw)
    marked = want["marked"]
    assert marked.sum() <= 0.02 * max(len(marked), 1) and not marked.any(), int(marked.sum())
    for k in INT_NAMES + ("cand",):
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(np.asarray(got[k]) != want[k])[0][:5])
    assert np.allclose(got["proj"], want["proj"], rtol=1e-12, atol=1e-9)
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["rot"], want["rot"])
    return got


SIZES = [(257, 300), (513, 768), (300, 1000), (64, 64)]
REASONS = [8260, 254, 501, 947, 1135, 303]            # searched, skip, behind, outside, range, angle
OUTCOMES = [3140, 3969, 2045, 1794, 9, 443]          # not searched, matched, no candidate, distance, ratio, orientation


def seeded(n_pt, n_kp):
    """the seeded scenes of one size: (sets, problems, L)"""
    out = []
    for direction in (-1, 0, 1):
        out.append(st.frame_scene(n_pt, n_kp, 100 + n_pt + direction, direction=direction, taken=direction == 0, skip=direction == 1) + (3,))
    for th, flags in ((1.0, False), (3.0, True)):
        out.append(st.local_scene(n_pt, n_kp, 200 + n_pt + int(th), th=th, taken=flags, skip=flags) + (3,))
    out.append(st.mixed_scene(3, n_pt, n_kp, 300 + n_pt) + (3,))
    out.append(st.frame_scene(n_pt, n_kp, 400 + n_pt, L=1) + (1,))
    out.append(st.local_scene(n_pt, n_kp, 500 + n_pt, L=1) + (1,))
    return out


@pytest.mark.parametrize("n_pt,n_kp", SIZES)
def test_seeded_scenes_in_both_modes(n_pt, n_kp):
    for sets, pbs, L in seeded(n_pt, n_kp):
        for p in pbs:
            assert 0.45 < (p["kp_ur"] >= 0).mean() < 0.75                 # right columns on about 60 % of the keypoints
        got = held(sets, pbs, L)
        assert (got["counts"][:, 1] > 0).all() and got["counts"][:, 0].sum() > 0


def test_crafted_scenes():
    for mode in (st.FRAME, st.LOCAL):
        got = held(*st.contention_scene(1, mode))
        assert (got["outcome"] == st.NO_CANDIDATE).sum() > 20 and got["counts"][0, 0] > 10       # several points want one keypoint
        got = held(*st.overflow_scene(2, mode))
        assert (got["n_cand"] > st.TOPK).all() and got["counts"][0, 2] == 40
    got = held(*st.ratio_scene(3))
    assert (got["outcome"] == st.RATIO).sum() >= 5 and got["counts"][0, 0] > 30
    open_ = held(*st.ratio_scene(3), ratio=1e300)
    assert (open_["outcome"] == st.RATIO).sum() == 0
    sets, pbs = st.frame_scene(513, 768, 3)
    got = held(sets, pbs)
    assert got["counts"][0, 3] >= 10 and (got["outcome"] == st.ORIENTATION).sum() == got["counts"][0, 3]
    off = held(sets, pbs, check_orientation=0)
    assert off["counts"][0, 3] == 0 and off["counts"][0, 0] == got["counts"][0, 0] + got["counts"][0, 3]
    # a removed match keeps its keypoint claimed: the matches that stay are the same with and without the check
    keep = got["match"] >= 0
    assert np.array_equal(got["match"][keep], off["match"][keep])
    held(sets, pbs, th_dist=40, baseline=0.3)
    held(*st.local_scene(257, 300, 9, th=3.0), ratio=0.6, r_near=1.5, r_wide=6.0, cos_near=0.9, th_dist=60)


def test_every_reason_and_outcome_occurs():
    """over the seeded scenes and the ratio scene, on the restatement: the counts DESIGN.md section 26 states"""
    reason, outcome = np.zeros(6, np.int64), np.zeros(6, np.int64)
    runs = [x for size in SIZES for x in seeded(*size)] + [st.ratio_scene(3) + (3,)]
    for sets, pbs, L in runs:
        got = st.search(sets, pbs, K4, W, H, L)
        reason += np.bincount(got["reason"], minlength=6)
        outcome += np.bincount(got["outcome"] + 1, minlength=6)
    reason, outcome = [int(x) for x in reason], [int(x) for x in outcome]
    assert list(reason) == REASONS and list(outcome) == OUTCOMES and min(REASONS) > 0 and min(OUTCOMES) > 0


@pytest.mark.parametrize("th", [3.0, 10.0])
def test_local_with_the_gate_open_is_the_projection_search(th):
    # few keypoints: the lists here are cut before the distance threshold, the projection search's after it, so they agree without overflow only
    for q, (n_pt, n_kp) in enumerate([(257, 64), (64, 100), (300, 80), (128, 120)]):
        sc = pr.scene(n_pt, n_kp, 70 + q, taken=q == 1, skip=q != 1)
        s, p = st.lf.split(sc)
        p.pop("kp_ur", None)
        p.update(mode=st.LOCAL, th=th, direction=0)
        got = st.search([s], [p], K4, W, H, 3, r_near=1.0, r_wide=1.0, ratio=1e300, th_dist=50)
        assert got["counts"][0, 2] == 0 and (got["n_cand"] <= st.TOPK).all()                      # no overflow
        ref = pr.search([sc], K4, th=th, th_dist=50, claim=1)
        assert np.array_equal(got["match"], ref["match"]) and np.array_equal(got["dist"], ref["dist"])
        assert np.array_equal(got["level"], ref["pred_level"]) and (got["match"] >= 0).sum() > 0


def test_orientation_is_the_oracles(oracle):
    for seed in (3, 4, 5):
        sets, pbs = st.frame_scene(513, 768, seed, turn=15.0 * seed)
        on, off = st.search(sets, pbs, K4, W, H, 3), st.search(sets, pbs, K4, W, H, 3, check_orientation=0)
        cnt, hist, ind = oracle.bow_orientation(sets[0]["pt_angle"], pbs[0]["kp_angle"], off["match"])
        assert cnt == on["counts"][0, 0] and list(on["rot"][0, :30]) == list(hist) and list(on["rot"][0, 30:]) == list(ind)
        assert on["counts"][0, 3] == off["counts"][0, 0] - cnt and on["counts"][0, 3] > 0


def test_what_the_right_column_buys():
    n = 2000
    sets, pbs = st.decoy_scene(n, 9, with_columns=False)
    assert set(np.unique(sets[0]["pt_level"])) == {0, 1, 2}
    got = st.search(sets, pbs, K4, W, H, 3)
    assert np.array_equal(got["match"], np.arange(n)) and (got["dist"] == 0).all()               # the decoy, for every point
    sets, pbs = st.decoy_scene(n, 9, with_columns=True)
    r = 7.0 * 2.0 ** sets[0]["pt_level"]
    off = np.abs(pbs[0]["kp_ur"][:n] - got["proj"][:, 2])
    assert (off > r + 0.5).all() and (off < r + 31).all()
    got = st.search(sets, pbs, K4, W, H, 3)
    assert np.array_equal(got["match"], np.arange(n) + n) and (got["dist"] == 5).all() and (got["n_gated"] >= 1).all()


def test_limits_and_defaults():
    L = st.lib()
    assert [L.st_limit(k) for k in range(4)] == [st.MAX_PROBLEMS, st.MAX_SETS, st.MAX_PAIRS, st.TOPK] == [64, 8, 262144, 8]
    p = st.default_params()
    assert [getattr(p, k) for k in st.PARAM_FIELDS] == [st.DEFAULTS[k] for k in st.PARAM_FIELDS] == [0.1, 0.8, 2.5, 4.0, 0.998, 100, 1]


# ---- the host rules on hand-made maps -------------------------------------------------------------------------------------------------------
def test_direction_rule():
    I = np.array([0, 0, 0, 1.0, 0, 0, 0])
    fwd, back, small = I.copy(), I.copy(), I.copy()
    fwd[6], back[6], small[6] = -0.25, 0.25, -0.05            # the camera moved 0.25 m forward: a world point is 0.25 m nearer
    assert st.direction(I, fwd, 0.1) == 1 and st.direction(I, back, 0.1) == -1 and st.direction(I, small, 0.1) == 0
    assert st.direction(I, fwd, 0.25) == 0 and st.direction(I, fwd, 0.1, has_columns=False) == 0
    q = np.array([0, np.sin(np.pi / 4), 0, np.cos(np.pi / 4)])            # both frames turned 90 degrees about y: the motion is along world x
    a, b = np.concatenate([q, [0, 0, 0]]), np.concatenate([q, [0, 0, -0.3]])
    assert st.direction(a, b, 0.1) == 1
    assert st.direction(np.concatenate([q, [0, 0, 1.0]]), np.concatenate([q, [0.3, 0, 1.0]]), 0.1) == 0     # sideways


def test_local_keyframes_rule():
    pts = {1: dict(bad=False, obs={2: 0, 5: 0}), 2: dict(bad=False, obs={5: 1, 7: 0}), 3: dict(bad=True, obs={9: 0}), 4: dict(bad=False, obs={7: 1, 2: 1})}
    kfs = {k: dict(bad=False, cov=[]) for k in (2, 5, 7, 8, 9, 11, 12)}
    kfs[7]["bad"] = True
    kfs[2]["cov"], kfs[5]["cov"], kfs[8]["cov"] = [5, 7, 8, 9], [2, 8, 11, 12], [12]
    out, ref = st.local_keyframes([1, None, 2, 3, 4], pts, kfs)
    # votes: 2 -> 2, 5 -> 2, 7 -> 2 (bad: votes but does not enter); the reference keyframe is the smallest id of the tie; 2's first free
    # neighbour is 8 (5 is in, 7 is bad), 5's is 11 (2 and 8 are in)
    assert out == [2, 5, 8, 11] and ref == 2
    out, _ = st.local_keyframes([1, 2, 4], pts, kfs, neighbours=2)
    assert out == [2, 5, 8]                                               # 2 looks at 5, 7 only: nothing; 5 at 2, 8
    out, _ = st.local_keyframes([1, 2, 4], pts, kfs, max_keyframes=3)
    assert out == [2, 5, 8]
    out, ref = st.local_keyframes([3, None], pts, kfs)
    assert out == [] and ref is None
    pts[2]["obs"][5] = 1; pts[4]["obs"][5] = 2
    assert st.local_keyframes([1, 2, 4], pts, kfs)[1] == 5               # most votes


def test_bookkeeping_rule():
    got = st.track_local_bookkeeping([1, 2], [3, 4, 5], [0, 3, 0], [7, -1, -1], [1, 3])
    assert got == {1: (1, 1, False), 2: (1, 0, False), 3: (1, 1, True), 4: (0, 0, False), 5: (1, 0, True)}
