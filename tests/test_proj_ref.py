"""tests/proj_ref.c, the restatement the device's projection-guided search is held to, against an independent numpy witness: brute force over
every (point, keypoint) pair, the level by np.ceil(np.log2(ratio)) as ORB-SLAM2's PredictScale writes it, and the claim as a naive
ORBmatcher::SearchByProjection loop that looks for the best unclaimed keypoint within the threshold.  The scenes keep every ratio 1e-6
relative away from a power of two and overflow no list (both asserted: they are conditions of the comparison); the overflow and the exact
powers of two have hand-built cases of their own."""
import numpy as np
import pytest

import proj_ref as pr

W, H, L = 640, 480, 3
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def witness(sc, th=10.0, th_dist=50, K4=pr.K4_DEFAULT):
    """-> reason [n], pred [n], per point the list of (dist, idx) of every candidate within th_dist, sorted"""
    S = np.asarray(sc["S"], float)
    R, t, s = pr.quat_to_R(S[:4]), S[4:7], S[7]
    n = len(sc["pt_dmax"])
    Xc = s * (np.asarray(sc["pw"]) @ R.T) + t
    reason, pred, cands, ratios = np.zeros(n, int), np.full(n, -1), [[] for _ in range(n)], np.full(n, np.nan)
    kp_px, kp_level = np.asarray(sc["kp_px"]), np.asarray(sc["kp_level"])
    free = np.ones(len(kp_level), bool) if sc.get("kp_taken") is None else np.asarray(sc["kp_taken"]) == 0
    for i in range(n):
        x, y, z = Xc[i]
        if sc.get("pt_skip") is not None and sc["pt_skip"][i]:
            reason[i] = pr.SKIP; continue
        if z <= 0:
            reason[i] = pr.BEHIND; continue
        u, v = K4[0] * x / z + K4[2], K4[1] * y / z + K4[3]
        if not (0 <= u < W and 0 <= v < H):
            reason[i] = pr.OUTSIDE; continue
        d = np.linalg.norm(Xc[i])
        dmax = sc["pt_dmax"][i]
        if d < 0.8 * dmax / 2 ** (L - 1) or d > 1.2 * dmax:
            reason[i] = pr.RANGE; continue
        if sc.get("pt_normal") is not None and Xc[i] @ (R @ sc["pt_normal"][i]) < 0.5 * d:
            reason[i] = pr.ANGLE; continue
        ratios[i] = dmax / d
        pred[i] = int(min(max(np.ceil(np.log2(ratios[i])), 0), L - 1))
        r = th * 2 ** pred[i]
        m = free & (np.abs(kp_px[:, 0] - u) < r) & (np.abs(kp_px[:, 1] - v) < r) & (kp_level >= pred[i] - 1) & (kp_level <= pred[i])
        for j in np.nonzero(m)[0]:
            dist = int(POP[np.bitwise_xor(sc["pt_desc"][i], sc["kp_desc"][j])].sum())
            if dist <= th_dist:
                cands[i].append((dist, int(j)))
        cands[i].sort()
    return reason, pred, cands, ratios


def naive_claim(cands, n_kp, claim):
    """ORB-SLAM2's loop: per point, in order, the best keypoint within the threshold that nobody took (ties: the smaller index)"""
    taken, match, dist = np.zeros(n_kp, bool), [], []
    for c in cands:
        best, bj = 10 ** 9, -1
        for d, j in c:
            if claim and taken[j]:
                continue
            if d < best or (d == best and j < bj):
                best, bj = d, j
        match.append(bj); dist.append(best if bj >= 0 else -1)
        if bj >= 0 and claim:
            taken[bj] = True
    return np.array(match), np.array(dist)


CASES = [dict(n_pt=300, n_kp=700, seed=1), dict(n_pt=257, n_kp=255, seed=2, s=1.2, taken=True, skip=True),
         dict(n_pt=200, n_kp=3072, seed=3, normals=False), dict(n_pt=400, n_kp=60, seed=4, taken=True), dict(n_pt=64, n_kp=1, seed=5, skip=True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "pt%d_kp%d" % (c["n_pt"], c["n_kp"]))
@pytest.mark.parametrize("th,th_dist", [(10.0, 50), (7.5, 100)])
def test_restatement_equals_the_numpy_witness(case, th, th_dist):
    sc = pr.scene(**case)
    reason, pred, cands, ratios = witness(sc, th, th_dist)
    ok = np.isfinite(ratios)
    frac = np.abs(np.log2(ratios[ok]) - np.round(np.log2(ratios[ok])))
    assert (frac > 2e-6).all(), "a ratio of the scene sits on a power of two"
    assert max([len(c) for c in cands]) <= pr.TOPK, "a list of the scene overflows"
    ref = pr.candidates(sc, th=th, th_dist=th_dist)
    assert np.array_equal(ref["reason"], reason)
    assert np.array_equal(ref["pred_level"], pred)
    assert np.array_equal(ref["n_cand"], [len(c) for c in cands])
    for i, c in enumerate(cands):
        k = len(c)
        assert [(int(d), int(j)) for d, j in zip(ref["cand_dist"][i, :k], ref["cand_idx"][i, :k])] == c, i
        assert (ref["cand_idx"][i, k:] == -1).all() and (ref["cand_dist"][i, k:] == -1).all()
    if len(sc["kp_level"]) > 1:
        assert len(set(reason)) >= 4 and sum(len(c) for c in cands) > len(cands) // 10      # the scene exercises the culls and finds candidates
    for claim in (0, 1):
        out = pr.search([sc], th=th, th_dist=th_dist, claim=claim)
        m, d = naive_claim(cands, len(sc["kp_level"]), claim)
        assert np.array_equal(out["match"], m) and np.array_equal(out["dist"], d)
        assert np.array_equal(out["pred_level"], pred)
        assert out["counts"].tolist() == [[int((m >= 0).sum()), 0]]
        if claim:
            hit = m[m >= 0]
            assert len(set(hit)) == len(hit)


def test_claim_has_contention_on_the_scenes():
    sc = pr.scene(400, 60, 4, taken=True)
    a, b = pr.search([sc], claim=0), pr.search([sc], claim=1)
    assert (a["match"] != b["match"]).any() and b["counts"][0, 0] < a["counts"][0, 0]


def _window_case(n_same, extra_dist=None):
    """one point straight ahead at the image centre's ray, n_same keypoints with its very descriptor inside the window"""
    K4 = pr.K4_DEFAULT
    rng = np.random.default_rng(9)
    desc = rng.integers(0, 256, 32).astype(np.uint8)
    kp_px = np.stack([K4[2] + np.linspace(-4, 4, n_same), np.full(n_same, K4[3])], 1)
    kp_desc = np.tile(desc, (n_same, 1))
    if extra_dist is not None:                         # the LAST keypoint is closer than all the others: it must still enter a full list
        kp_desc[:-1] = pr.flip_bits(rng, desc, extra_dist)
    return dict(kp_px=kp_px, kp_level=np.zeros(n_same, np.int32), kp_desc=kp_desc, pw=[[0, 0, 4.0]], pt_desc=[desc], pt_dmax=[4.0],
                S=[0, 0, 0, 1, 0, 0, 0, 1.0])


def test_nine_equal_descriptors_overflow_and_truncate():
    sc = _window_case(9)
    ref = pr.candidates(sc)
    assert ref["n_cand"][0] == 9 and ref["cand_idx"][0].tolist() == list(range(8)) and (ref["cand_dist"][0] == 0).all()
    out = pr.search([sc, sc], claim=1)
    assert out["match"].tolist() == [0, 0] and out["counts"].tolist() == [[1, 1], [1, 1]]
    sc = _window_case(9, extra_dist=5)
    ref = pr.candidates(sc)
    assert ref["n_cand"][0] == 9 and ref["cand_idx"][0].tolist() == [8, 0, 1, 2, 3, 4, 5, 6] and ref["cand_dist"][0].tolist() == [0] + [5] * 7
    # two such points, claim on: the second takes the next entry; a point whose eight entries are all taken gets nothing although a ninth
    # candidate exists -- the truncation the specification accepts
    two = dict(_window_case(9), pw=[[0, 0, 4.0]] * 10, pt_desc=np.tile(_window_case(9)["pt_desc"], (10, 1)), pt_dmax=[4.0] * 10)
    out = pr.search([two], claim=1)
    assert out["match"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, -1] and out["counts"].tolist() == [[8, 10]]


@pytest.mark.parametrize("ratio,level", [(1.0, 0), (2.0, 1), (4.0, 2)])
def test_exact_powers_of_two(ratio, level):
    sc = _window_case(1)
    sc["pt_dmax"] = [4.0 * ratio]
    ref = pr.candidates(sc)
    assert ref["reason"][0] == pr.KEPT and ref["pred_level"][0] == level
    sc["pt_dmax"] = [np.nextafter(4.0 * ratio, np.inf)]
    assert pr.candidates(sc)["pred_level"][0] == min(level + 1, L - 1)
