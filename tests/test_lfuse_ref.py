"""The restatement of the local-map fusion search (tests/lfuse_ref.c) held to a numpy witness written another way: brute
force over all keypoints, the predicted level as np.ceil(np.log2(ratio)), the gate as e2 / 4^level > chi2, the rotation as a matrix product.
match, dist, reason and n_gated are EQUAL for every point the witness does not mark as within 1e-9 relative of a threshold; the seeds mark none
(asserted here).  Also: every reason and gated candidates on mono and on stereo keypoints occur; with both chi2 at 1e300 and no right column
the call is proj_ref.search(claim=0, S=(q, t, 1)) exactly; what the uR term buys on the decoy scene; the Python restatement of
StereoMapper::SearchInNeighbors' walk and of MapPointCulling's rule on hand-made maps."""
import numpy as np
import pytest

import lfuse_ref as lf
import proj_ref as pr

EPS = 1e-9
SCENES = [(257, 300, 11), (513, 768, 12), (300, 1000, 13), (64, 64, 14)]       # n_pt, n_kp, seed
# the decoy scene (seed 5, 2000 points): acceptance rate with kp_ur = -1 and with the columns, on the restatement; the test's threshold lies
# between them
DECOY_RATE_MONO, DECOY_RATE_STEREO, DECOY_THRESHOLD = 1.0, 0.136, 0.55


def near(a, b, scale=None):
    return abs(a - b) <= EPS * (abs(b) if scale is None else scale)


def witness(sets, problems, K4=lf.K4_DEFAULT, w=640, h=480, L=3, **kw):
    """match, dist, pred_level, reason, n_gated [N], and marked [N]: the point is within 1e-9 relative of one of its thresholds"""
    prm = dict(lf.DEFAULTS, **kw)
    bf = K4[0] * prm["baseline"]
    out = {k: [] for k in ("match", "dist", "pred_level", "reason", "n_gated", "marked", "gated_mono", "gated_stereo")}
    for pb in problems:
        s = sets[pb.get("set", 0)]
        pw, desc, dmax = np.asarray(s["pw"]).reshape(-1, 3), np.asarray(s["pt_desc"], np.uint8).reshape(-1, 32), np.asarray(s["pt_dmax"]).reshape(-1)
        nrm = np.asarray(s["pt_normal"]).reshape(-1, 3) if s.get("pt_normal") is not None else None
        T = np.asarray(pb["T"], np.float64)
        R, t = pr.quat_to_R(T[:4]), T[4:7]
        kp_px, kp_level = np.asarray(pb["kp_px"]).reshape(-1, 2), np.asarray(pb["kp_level"]).reshape(-1)
        kp_bits = np.unpackbits(np.asarray(pb["kp_desc"], np.uint8).reshape(-1, 32), axis=1)
        n_kp = len(kp_level)
        kur = np.asarray(pb["kp_ur"]).reshape(-1) if pb.get("kp_ur") is not None else np.full(n_kp, -1.0)
        free = np.ones(n_kp, bool) if pb.get("kp_taken") is None else np.asarray(pb["kp_taken"]).reshape(-1) == 0
        skip = pb.get("pt_skip")
        for i in range(len(dmax)):
            m, dd, pred, why, ng, mark, gm, gs = -1, -1, -1, lf.SEARCHED, 0, False, 0, 0
            X = R @ pw[i] + t
            d = float(np.linalg.norm(X))
            if skip is not None and skip[i]:
                why = lf.SKIP
            elif not X[2] > 0:
                why = lf.BEHIND
            else:
                mark |= near(X[2], 0.0, max(d, 1e-300))
                u, v = K4[0] * X[0] / X[2] + K4[2], K4[1] * X[1] / X[2] + K4[3]
                mark |= near(u, 0, w) or near(u, w) or near(v, 0, h) or near(v, h)
                dmin = dmax[i] / 2.0 ** (L - 1)
                if not (0 <= u < w and 0 <= v < h):
                    why = lf.OUTSIDE
                elif d < 0.8 * dmin or d > 1.2 * dmax[i]:
                    why = lf.RANGE
                    mark |= near(d, 0.8 * dmin) or near(d, 1.2 * dmax[i])
                elif nrm is not None and float(X @ (R @ nrm[i])) < 0.5 * d:
                    why = lf.ANGLE
                    mark |= near(float(X @ (R @ nrm[i])), 0.5 * d)
                else:
                    mark |= near(d, 0.8 * dmin) or near(d, 1.2 * dmax[i])
                    if nrm is not None:
                        mark |= near(float(X @ (R @ nrm[i])), 0.5 * d)
                    ratio = dmax[i] / d
                    lg = np.log2(ratio)
                    mark |= abs(lg - np.round(lg)) <= 4 * EPS
                    pred = int(np.clip(np.ceil(lg), 0, L - 1))
                    r = prm["th"] * 2.0 ** pred
                    ur = u - bf / X[2]
                    dx, dy = np.abs(kp_px[:, 0] - u), np.abs(kp_px[:, 1] - v)
                    lvl = free & (kp_level >= pred - 1) & (kp_level <= pred)
                    mark |= bool((lvl & ((np.abs(dx - r) <= EPS * r) | (np.abs(dy - r) <= EPS * r))).any())
                    win = lvl & (dx < r) & (dy < r)
                    stereo = kur >= 0
                    e2 = (u - kp_px[:, 0]) ** 2 + (v - kp_px[:, 1]) ** 2 + np.where(stereo, (ur - kur) ** 2, 0.0)
                    chi = np.where(stereo, prm["chi2_stereo"], prm["chi2_mono"])
                    q = e2 / 4.0 ** np.clip(kp_level, 0, 30)
                    mark |= bool((win & (np.abs(q - chi) <= EPS * chi)).any())
                    gated = win & (q > chi)
                    ng, gm, gs = int(gated.sum()), int((gated & ~stereo).sum()), int((gated & stereo).sum())
                    ok = np.flatnonzero(win & ~gated)
                    if len(ok):
                        ham = (kp_bits[ok] != np.unpackbits(desc[i])[None, :]).sum(1)
                        k = int(np.lexsort((ok, ham))[0])
                        if ham[k] <= prm["th_dist"]:
                            m, dd = int(ok[k]), int(ham[k])
            for k, val in zip(out, (m, dd, pred, why, ng, mark, gm, gs)):
                out[k].append(val)
    return {k: np.array(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def scenes():
    """the seeded scenes, each once: (sets, problems, restatement, witness)"""
    out = []
    for n_pt, n_kp, seed in SCENES:
        sc = lf.scene(n_pt, n_kp, seed, taken=seed % 2 == 0, skip=True)
        s, p = lf.split(sc)
        out.append(([s], [p], lf.search([s], [p]), witness([s], [p])))
    return out


def test_restatement_equals_the_witness(scenes):
    seen, gm, gs, matched, marked = np.zeros(6, np.int64), 0, 0, 0, 0
    for (n_pt, n_kp, seed), (sets, pbs, got, want) in zip(SCENES, scenes):
        ok = ~want["marked"].astype(bool)
        marked += int((~ok).sum())
        assert (~ok).sum() <= 0.02 * n_pt
        for k in ("match", "dist", "reason", "n_gated", "pred_level"):
            assert np.array_equal(got[k][ok], want[k][ok]), (seed, k)
        assert got["counts"][0, 0] == (got["match"] >= 0).sum() and got["counts"][0, 1] == (got["reason"] == 0).sum()
        seen += np.bincount(got["reason"], minlength=6)
        gm, gs, matched = gm + want["gated_mono"].sum(), gs + want["gated_stereo"].sum(), matched + (got["match"] >= 0).sum()
    assert marked == 0                                                  # the seeds mark no point: every point of every scene is compared
    assert (seen > 0).all(), seen                                       # every reason 0-5 occurs
    assert gm > 0 and gs > 0 and matched > 20, (gm, gs, matched)


def test_other_parameters_and_no_normals():
    sc = lf.scene(200, 257, 21, normals=False, L=4, taken=True)
    s, p = lf.split(sc)
    kw = dict(th=5.0, th_dist=70, baseline=0.25, chi2_mono=3.0, chi2_stereo=20.0)
    got, want = lf.search([s], [p], L=4, **kw), witness([s], [p], L=4, **kw)
    assert not want["marked"].any()
    for k in ("match", "dist", "reason", "n_gated", "pred_level"):
        assert np.array_equal(got[k], want[k]), k
    assert not (got["reason"] == lf.ANGLE).any()


def test_two_sets_and_interleaved_problems():
    a, pa = lf.shared_scene(65, 100, 2, 31)
    b, pb = lf.shared_scene(130, 90, 1, 32)
    sets = [a[0], b[0]]
    pbs = [dict(pa[0], set=0), dict(pb[0], set=1), dict(pa[1], set=0)]
    got, want = lf.search(sets, pbs), witness(sets, pbs)
    assert list(lf.offsets(sets, pbs)) == [0, 65, 195, 260] and len(got["match"]) == 260
    ok = ~want["marked"].astype(bool)
    assert ok.all()
    for k in ("match", "dist", "reason", "n_gated", "pred_level"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["match"] >= 0).sum() > 10


def test_open_gate_is_the_projection_search(scenes):
    for (n_pt, n_kp, seed), (sets, pbs, _, _) in zip(SCENES, scenes):
        p = {k: v for k, v in pbs[0].items() if k != "kp_ur"}
        for th in (3.0, 10.0):
            got = lf.search(sets, [p], th=th, chi2_mono=1e300, chi2_stereo=1e300)
            S = np.concatenate([p["T"], [1.0]])
            ref = pr.search([dict(sets[0], S=S, **{k: v for k, v in p.items() if k not in ("T", "set")})], claim=0, th=th, th_dist=50)
            for k in ("match", "dist", "pred_level"):
                assert np.array_equal(got[k], ref[k]), (seed, th, k)
            assert (got["n_gated"] == 0).all()
        assert (ref["match"] >= 0).sum() > 0


def decoy_rates(search, n=2000, seed=5):
    rates = []
    for cols in (False, True):
        sets, pbs = lf.decoy_scene(n, seed, with_columns=cols)
        got = search(sets, pbs)
        assert (got["reason"] == 0).all()
        rates.append(float((got["match"] == np.arange(n)).mean()))
    return rates


def test_what_the_right_column_buys():
    mono, stereo = decoy_rates(lf.search)
    print("decoy acceptance: kp_ur = -1 %.4f, with the columns %.4f" % (mono, stereo))
    assert abs(mono - DECOY_RATE_MONO) < 5e-4 and abs(stereo - DECOY_RATE_STEREO) < 5e-4
    assert stereo < DECOY_THRESHOLD < mono


# ---- the walk and the culling rule on hand-made maps -----------------------------------------------------------------------------------------
def hand_map():
    """keyframes 0 (current), 1, 2; features: stereo flags make nObs differ.  Points: 10, 11 seen by kf 0; 20 by kf 1 (stereo) and kf 2; 21 by
    kf 1 (mono); 22 bad, still named by kf 2's feature 2; 23 by kf 2"""
    pt = lambda obs, bad=False, fs=0: dict(bad=bad, obs=obs, cnt_found=1, cnt_visible=1, first_seen=fs)
    points = {10: pt({0: 0}), 11: pt({0: 1}), 12: pt({0: 2}), 20: pt({1: 0, 2: 0}), 21: pt({1: 1}), 22: pt({2: 2}, bad=True), 23: pt({2: 3})}
    features = {0: [10, 11, 12, -1], 1: [20, 21, -1], 2: [20, -1, 22, 23]}
    stereo = {0: [True, False, False, False], 1: [True, False, False], 2: [False, False, False, False]}
    return lf.make_map(points, features, stereo)


def consistent(m):
    for k, fs in m["features"].items():
        for f, pid in enumerate(fs):
            if pid >= 0 and not m["points"][pid]["bad"]:
                assert m["points"][pid]["obs"].get(k) == f
    for pid, p in m["points"].items():
        for k, f in p["obs"].items():
            if not p["bad"]:
                assert m["features"][k][f] == pid


def test_walk_on_a_hand_made_map():
    m = hand_map()
    touched = set()
    hits = [(1, 10, 0),     # q = 20 has nObs 3 > nObs(10) = 2: 10 is replaced by 20
            (1, 11, 1),     # q = 21 nObs 1 = nObs(11) 1: a tie, 21 is replaced by 11
            (1, 12, 2),     # free feature: added
            (2, 10, 0),     # 10 -> 20 by now, and 20 is observed by 2: conflict
            (2, 11, 2),     # the feature names the bad 22: added, 22 loses the observation
            (2, 12, 3),     # q = 23 nObs 1 < nObs(12) = 2: 23 replaced by 12
            (2, 12, 1)]     # 12 is observed by 2 now: conflict
    acts = lf.walk(m, hits, touched)
    assert acts == [(lf.REPLACED_INTO_FEATURE, 1, 10, 0, 20), (lf.REPLACED_INTO_POINT, 1, 11, 1, 11), (lf.ADDED, 1, 12, 2, 12),
                    (lf.CONFLICT, 2, 10, 0, 20), (lf.ADDED, 2, 11, 2, 11), (lf.REPLACED_INTO_POINT, 2, 12, 3, 12), (lf.CONFLICT, 2, 12, 1, 12)]
    assert m["points"][10]["bad"] and m["points"][21]["bad"] and m["points"][23]["bad"] and m["features"][0][0] == 20
    assert m["points"][20]["obs"] == {0: 0, 1: 0, 2: 0} and m["points"][11]["obs"] == {0: 1, 1: 1, 2: 2} and m["points"][22]["obs"] == {}
    assert m["points"][12]["obs"] == {0: 2, 1: 2, 2: 3} and m["points"][20]["cnt_found"] == 2
    assert touched == {0, 1, 2}
    consistent(m)
    # q == P: nothing, not even an action
    assert lf.walk(m, [(1, 11, 1)]) == [(lf.CONFLICT, 1, 11, 1, 11)]       # already observed by 1 comes first


def test_culling_rule_on_a_hand_made_list():
    pt = lambda obs, found, visible, fs, bad=False: dict(bad=bad, obs=obs, cnt_found=found, cnt_visible=visible, first_seen=fs)
    points = {1: pt({}, 1, 1, 5, bad=True),                 # bad: dropped
              2: pt({5: 0}, 1, 5, 7),                       # found ratio 0.2 < 0.25: killed
              3: pt({5: 1, 6: 0}, 3, 4, 5),                 # c = 7 >= 5 + 2 and nObs = 2 <= 3: killed
              4: pt({5: 2, 6: 1, 7: 0}, 3, 4, 4),           # nObs 4 (stereo in 7), c >= 4 + 3: survived, dropped from the list
              5: pt({6: 2, 7: 1}, 3, 4, 6),                 # too young for either: stays
              6: pt({7: 2}, 0, 0, 7),                       # _cnt_visible = 0: no ratio; young: stays
              7: pt({5: 3, 6: 3}, 1, 4, 5)}                 # ratio exactly 0.25 is not below it; stereo in 6: nObs 3 <= 3 killed
    features = {5: [2, 3, 4, 7], 6: [3, 4, 5, 7], 7: [4, 5, 6]}
    stereo = {5: [False] * 4, 6: [False, False, False, True], 7: [True, False, False]}
    m = lf.make_map(points, features, stereo)
    keep, dead = lf.cull(m, [1, 2, 3, 4, 5, 6, 7], 7)
    assert keep == [5, 6] and dead == [2, 3, 7]
    assert m["features"] == {5: [-1, -1, 4, -1], 6: [-1, 4, 5, -1], 7: [4, 5, 6]}
    m2 = lf.make_map(points, features, stereo)
    keep, dead = lf.cull(m2, [7, 3], 7, min_obs=2)                              # the mono caller's value: 3 > 2 observations survive
    assert keep == [7] and dead == [3]
