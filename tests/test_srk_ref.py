"""The definition of the stereo reference-keyframe tracking on resident slots (tests/srk_ref.py) on exact synthetic
arrays, without an image and without a GPU: the joining formulas against a second writing, element by element, and one exact scene against its
truth.

Measured on the exact scene (300 world points 8 .. 20 m in front of the keyframe, keyframe and frame keypoints their exact projections with
exact depths, each pair sharing a random descriptor, tests/bow_cases.ragged_vocabulary() at levelsup 1, seed 3, T the truth turned by 0.09
degrees of yaw and moved by 1 mm): 271 of the 300 descriptors land in the FeatureVector (the rest hit stopped words), every one of them matches
its twin and nothing else, in 13 distinct nodes; 271 edges, no outlier, four rounds.  The largest |T_out - truth| over the seven components is
1.11e-16 (the translation); the test asserts ten times that, 1.11e-15."""
import numpy as np
import pytest

import bow_cases as bc
import popt_ref
import srk_ref as sk

K = popt_ref.DEFAULT_K
T_OUT_MEASURED = 1.11e-16
T_OUT_BOUND = 10 * T_OUT_MEASURED


def perturbed(a=0.0008, dx=0.001):
    return sk.se3_mul(np.array([0, np.sin(a), 0, np.cos(a), dx, 0, 0]), sk.TRUTH)


@pytest.fixture(scope="module")
def vocab():
    return sk.oracle().vocab_parse(bc.ragged_vocabulary())


def test_masking_of_node1():
    node = np.array([5, 7, -1, 9, 9, 0], np.int32)
    kfp = np.array([3, -1, 2, -1, 0, 0], np.int32)
    got = sk.masked_nodes(node, kfp)
    assert got.dtype == np.int32 and got.tolist() == [node[i] if kfp[i] >= 0 else -1 for i in range(6)] == [5, -1, -1, -1, 9, 0]


def test_masked_feature_is_not_searched(vocab):
    """a keyframe feature without a point matches nothing, and takes nothing from the others: the search treats every row on its own"""
    rng = np.random.default_rng(5)
    d = bc.vocabulary_features(bc.ragged_vocabulary(), 80, 6)
    fr = dict(px=rng.uniform(20, 300, (80, 2)), level=np.zeros(80, np.int32), angle=np.zeros(80, np.float32), desc=d, depth=np.full(80, 4.0),
              has_mp=np.ones(80, np.uint8))
    kfp = np.arange(80, dtype=np.int32)
    kfp[::3] = -1
    s = dict(pw=rng.uniform(-1, 1, (80, 3)) + [0, 0, 6])
    full = sk.track_frame(fr, fr, np.arange(80), s, sk.IDENTITY, vocab, levelsup=1, min_matches=1000)
    part = sk.track_frame(fr, fr, kfp, s, sk.IDENTITY, vocab, levelsup=1, min_matches=1000)
    assert (part["found"][::3] == -1).all() and (part["outcome"][::3] == -1).all() and (part["node1"][::3] == -1).all()
    keep = kfp >= 0
    assert np.array_equal(part["found"][keep], full["found"][keep]) and (full["found"] >= 0).sum() > 40
    assert part["counts"][1] == keep.sum() and part["status"] == 1 and part["T_out"].tobytes() == sk.IDENTITY.tobytes()


def test_claim_with_three_features_on_one_keypoint():
    match = np.array([4, -1, 2, 4, 0, 4, 2, -1], np.int32)
    holder, lost = sk.claim(match, 6)
    assert holder.tolist() == [4, -1, 2, -1, 0, -1] and lost.tolist() == [False, False, False, True, False, True, True, False]
    # a second writing: per keypoint the minimum over the features that name it
    for j in range(6):
        who = np.flatnonzero(match == j)
        assert holder[j] == (who.min() if len(who) else -1)
        assert all(lost[i] == (i != who.min()) for i in who)
    kfp = np.array([10, 11, 12, 13, 14, 15, 12, 17], np.int32)         # features 2 and 6 carry the same point
    kp_point = sk.keypoint_points(np.where(lost, -1, match), kfp, 6)
    assert kp_point.tolist() == [14, -1, 12, -1, 10, -1]


@pytest.mark.parametrize("rot, want", [(14.75, 0), (15.0, 1), (15.25, 1), (359.75, 12), (45.0, 2), (75.0, 3), (0.0, 0), (-0.25, 12)])
def test_rotation_bin_rounds_half_away_from_zero(rot, want):
    """round(15 / 30) and round(75 / 30) are 1 and 3 in C; numpy's round gives 0 and 2"""
    a2 = np.array([10.0], np.float32)
    a1 = np.array([10.0 + rot], np.float32)
    b = sk.rotation_bins(a1, a2, np.array([0], np.int32))
    _, hist, _ = sk.oracle().bow_orientation(a1.astype(np.float64), a2.astype(np.float64), np.array([0], np.int32))
    assert b[0] == want and hist[want] == 1 and hist.sum() == 1


def test_orientation_removal_at_the_bin_edges():
    """matches in bin 0 and one each at 14.75 (bin 0), 15 and 15.25 (bin 1) and 359.75 degrees (bin 12): with 13 in bin 0 the 2 of bin 1 are
    a tenth and stand, bin 12 goes; with 31 in bin 0 only that bin stands and the three others are removed"""
    rots = [1.0] * 12 + [14.75, 15.0, 15.25, 359.75]
    n = len(rots)
    a2 = np.linspace(0, 300, n).astype(np.float32)
    a1 = ((a2.astype(np.float64) + rots) % 360.0).astype(np.float32)
    match = np.arange(n, dtype=np.int32)
    hist, ind, removed = sk.orientation(a1, a2, match)
    assert hist[0] == 13 and hist[1] == 2 and hist[12] == 1 and hist.sum() == n and ind.tolist() == [0, 1, -1]
    assert np.flatnonzero(removed).tolist() == [15]                       # 2 is not below 0.1f * 13, so bin 1 stands; bin 12 goes
    # with 30 matches in bin 0 the second bin falls below a tenth
    rots = [1.0] * 30 + [14.75, 15.0, 15.25, 359.75]
    n = len(rots)
    a2 = np.linspace(0, 300, n).astype(np.float32)
    a1 = ((a2.astype(np.float64) + rots) % 360.0).astype(np.float32)
    hist, ind, removed = sk.orientation(a1, a2, np.arange(n, dtype=np.int32))
    assert hist[0] == 31 and ind.tolist() == [0, -1, -1] and np.flatnonzero(removed).tolist() == [31, 32, 33]
    # the histogram against the bins, element by element; unmatched rows are in neither
    m = np.arange(n, dtype=np.int32)
    m[::4] = -1
    hist, ind, removed = sk.orientation(a1, a2, m)
    bins = sk.rotation_bins(a1, a2, m)
    assert (bins[::4] == -1).all() and not removed[::4].any() and np.array_equal(hist, np.bincount(bins[bins >= 0], minlength=30))


def test_edge_order_and_prior():
    rng = np.random.default_rng(3)
    n2, n_pt = 40, 30
    px = np.stack([rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)], 1)
    depth = rng.uniform(-1, 10, n2)
    depth[::7] = np.nan
    has_mp = (rng.uniform(size=n2) < 0.8).astype(np.uint8)
    ur = sk.right_columns(px, depth, sk.has_depth(depth, has_mp), 0.1, K)
    match = np.full(25, -1, np.int32)
    match[[20, 3, 9, 14, 0]] = [5, 31, 7, 0, 38]                        # keyframe feature -> frame keypoint, not in keypoint order
    kfp = rng.permutation(n_pt)[:25].astype(np.int32)
    kp_point = sk.keypoint_points(match, kfp, n2)
    want = {5: kfp[20], 31: kfp[3], 7: kfp[9], 0: kfp[14], 38: kfp[0]}
    assert {int(j): int(kp_point[j]) for j in np.flatnonzero(kp_point >= 0)} == {k: int(v) for k, v in want.items()}
    pw = rng.uniform(-5, 5, (n_pt, 3))
    lvl = rng.integers(0, 3, n2).astype(np.int32)
    j, X, obs, level, kind = sk.edges(kp_point, pw, px, ur, lvl)
    assert j.tolist() == [0, 5, 7, 31, 38]                               # j ascending: PoseOptimizer::Optimize's order
    for e, jj in enumerate(j):
        assert (X[e] == pw[want[jj]]).all() and obs[e].tolist() == [px[jj, 0], px[jj, 1], ur[jj]] and level[e] == lvl[jj]
        assert kind[e] == (2 if ur[jj] >= 0 else 1)
    outlier = np.zeros(n2, np.uint8)
    outlier[[5, 38]] = 1
    prior = sk.prior_of(kp_point, outlier)
    assert prior.dtype == np.int32 and [int(prior[q]) for q in (0, 5, 7, 31, 38)] == [int(want[0]), -1, int(want[7]), int(want[31]), -1]
    assert (prior[kp_point < 0] == -1).all()


@pytest.fixture(scope="module")
def tracked(vocab):
    kfr, fr, s = sk.exact_scene()
    return (kfr, fr, s), sk.track_frame(kfr, fr, np.arange(300), s, perturbed(), vocab, levelsup=1)


def test_exact_scene(tracked):
    (kfr, fr, s), o = tracked
    n = 300
    inside = o["node1"] >= 0
    print("in the FeatureVector %d of %d, distinct nodes %d, edges %d" % (inside.sum(), n, len(np.unique(o["node1"][inside])), o["counts"][7]))
    assert np.array_equal(o["match12"][inside], np.flatnonzero(inside)) and (o["match12"][~inside] == -1).all()
    assert o["counts"][7] >= 250 and len(np.unique(o["node1"][inside])) >= 8
    assert o["counts"].tolist() == [n, n, n, n, inside.sum(), 0, 0, inside.sum()] and o["status"] == 0
    assert not o["outlier"].any() and o["inliers"] == inside.sum() and o["rounds_run"] == 4
    assert np.array_equal(o["prior"], o["kp_point"]) and np.array_equal(np.flatnonzero(o["kp_point"] >= 0), np.flatnonzero(inside))
    assert o["rot"][0] == inside.sum() and o["rot"][30:].tolist() == [0, -1, -1]
    err = np.abs(o["T_out"] - sk.TRUTH).max()
    print("max |T_out - truth| = %.3e (measured %.3e, bound %.3e)" % (err, T_OUT_MEASURED, T_OUT_BOUND))
    assert err <= T_OUT_BOUND


def test_too_few_matches_and_too_few_inliers(tracked, vocab):
    (kfr, fr, s), o = tracked
    T0 = perturbed()
    few = sk.track_frame(kfr, fr, np.arange(300), s, T0, vocab, levelsup=1, min_matches=1000)
    assert few["status"] == 1 and few["T_out"].tobytes() == T0.tobytes() and not few["outlier"].any() and (few["chi2"] == -1.0).all()
    assert np.array_equal(few["kp_point"], o["kp_point"]) and np.array_equal(few["prior"], few["kp_point"]) and few["inliers"] == 0
    low = sk.track_frame(kfr, fr, np.arange(300), s, T0, vocab, levelsup=1, min_inliers=1000)
    assert low["status"] == 2 and low["T_out"].tobytes() == o["T_out"].tobytes()
    none = sk.track_frame(kfr, fr, np.full(300, -1), s, T0, vocab, levelsup=1)
    assert none["status"] == 1 and none["counts"].tolist() == [300, 0, 300, 300, 0, 0, 0, 0] and (none["outcome"] == -1).all()
    assert none["T_out"].tobytes() == T0.tobytes()


def test_joined_outputs_and_limits(tracked):
    (kfr, fr, s), o = tracked
    j = sk.joined([o, o], 400)
    assert j["kp_point"].shape == (2, 400) and (j["kp_point"][:, 300:] == -1).all() and (j["chi2"][:, 300:] == -1.0).all()
    assert (j["match12"][:, 300:] == -1).all() and (j["outcome"][:, 300:] == -1).all() and not j["outlier"][:, 300:].any()
    assert j["rot"].shape == (2, 33) and j["T_out"].shape == (2, 7) and j["counts"].shape == (2, 8)
    assert sk.MAX_FRAMES == 1024 and sk.MAX_KEYFRAMES == 256 and sk.MAX_SETS == 64
