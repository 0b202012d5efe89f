"""The definition of the stereo local-map tracking on resident slots (tests/slm_ref.py) on exact synthetic arrays,
without an image and without a GPU: the joining formulas against a second writing, the exact scene against its truth, and the crafted frames
(a prior that covers 100 keypoints, the ratio rule, contention, two edges, an empty set with a prior).

Measured on the exact scene (300 points 8 .. 20 m in front of the camera, the keypoints their exact projections with exact depths, T the
truth turned by 0.09 degrees of yaw and moved by 1 mm, so that every projection is off by up to 1.1 px, inside the 2.5 px LOCAL window at th
1): the largest |T_out - truth| over the seven components is 5.00e-16 (the translation's z; the quaternion is off by less than 3e-17).  The
test asserts ten times that, 5.00e-15."""
import numpy as np
import pytest

import popt_ref
import slm_ref as sl
import strack_ref

K = popt_ref.DEFAULT_K
T_OUT_MEASURED = 5.00e-16
T_OUT_BOUND = 10 * T_OUT_MEASURED


def perturbed(a=0.0008, dx=0.001):
    return sl.se3_mul(np.array([0, np.sin(a), 0, np.cos(a), dx, 0, 0]), sl.TRUTH)


@pytest.fixture(scope="module")
def scene():
    return sl.exact_scene()


@pytest.fixture(scope="module")
def tracked(scene):
    return sl.track_frame(scene[0], scene[1], perturbed())


def test_formulas_against_a_second_writing():
    rng = np.random.default_rng(3)
    n, n_pt = 200, 150
    px = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)
    depth = rng.uniform(-1, 10, n)
    depth[::17] = np.nan                                               # NaN depths
    depth[5] = 0.0
    has_mp = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    has_mp[8], depth[8] = 0, 3.0                                       # a flag of 0 with a depth
    has_mp[9], depth[9] = 1, 3.0
    bf = K[0] * 0.1
    ur = sl.right_columns(px, depth, sl.has_depth(depth, has_mp), 0.1, K)
    for j in range(n):
        d = float(depth[j])
        if bool(has_mp[j]) and not np.isnan(d) and d > 0:
            assert ur[j] == float(px[j, 0]) - bf / d
        else:
            assert ur[j] == -1.0
    assert ur[8] == -1.0 and ur[9] >= 0 and (ur[::17] == -1.0).all()
    # the prior: duplicates (keypoints 3 and 40 name point 7), a prior on a keypoint without depth (8), entries past n_kp ignored
    prior = np.full(n + 20, -1, np.int32)
    prior[[3, 40, 8, 11, 150]] = [7, 7, 20, 0, 149]
    prior[n + 3] = 5
    pr, taken, skip = sl.prior_flags(prior, n, n_pt)
    assert len(pr) == n and np.flatnonzero(taken).tolist() == [3, 8, 11, 40, 150] and np.flatnonzero(skip).tolist() == [0, 7, 20, 149]
    none = sl.prior_flags(None, n, n_pt)
    assert (none[0] == -1).all() and not none[1].any() and not none[2].any()
    # the point a keypoint ends with, and the edge order with prior and new edges interleaved
    match = np.full(n_pt, -1)
    match[[2, 9, 100, 148]] = [60, 5, 4, 199]                          # point -> keypoint
    kp_point = sl.keypoint_points(pr, match)
    want = {3: 7, 4: 100, 5: 9, 8: 20, 11: 0, 40: 7, 60: 2, 150: 149, 199: 148}
    assert {int(j): int(kp_point[j]) for j in np.flatnonzero(kp_point >= 0)} == want
    pw = rng.uniform(-5, 5, (n_pt, 3))
    kp_level = rng.integers(0, 3, n).astype(np.int32)
    j, X, obs, lvl, kind = sl.edges(kp_point, pw, px, ur, kp_level)
    assert j.tolist() == sorted(want)                                   # keypoint order: 3 (prior), 4, 5 (new), 8 (prior) ...
    for e, jj in enumerate(sorted(want)):
        assert (X[e] == pw[want[jj]]).all() and obs[e].tolist() == [px[jj, 0], px[jj, 1], ur[jj]] and lvl[e] == kp_level[jj]
        assert kind[e] == (2 if ur[jj] >= 0 else 1)
    assert kind[sorted(want).index(8)] == 1                            # the prior on a keypoint without depth is a mono edge
    assert (X[sorted(want).index(3)] == X[sorted(want).index(40)]).all()      # both duplicates are edges of the same point


def test_exact_scene_matches_every_point(scene, tracked):
    fr, s = scene
    o, n = tracked, len(scene[0]["level"])
    off = np.abs(o["proj"][:, :2] - fr["px"]).max(1)
    assert off.min() > 0.3 and off.max() < 2.0                          # T is off, and every projection is inside the 2.5 px window
    assert o["status"] == 0 and o["counts"].tolist() == [n, n, 0, n, n, 0, n, n]
    assert np.array_equal(o["match"], np.arange(n)) and (o["dist"] == 0).all() and (o["outcome"] == strack_ref.MATCHED).all()
    assert np.array_equal(o["kp_point"], np.arange(n)) and (o["reason"] == strack_ref.SEARCHED).all()
    assert o["inliers"] == n and not o["outlier"].any() and (o["chi2"] >= 0).all() and o["rounds_run"] == 4
    err = np.abs(o["T_out"] - sl.TRUTH).max()
    print("max |T_out - truth| = %.3e (measured %.3e, bound %.3e)" % (err, T_OUT_MEASURED, T_OUT_BOUND))
    assert err <= T_OUT_BOUND


def test_prior_covering_100_keypoints(scene, tracked):
    fr, s = scene
    n = len(fr["level"])
    prior = np.full(n, -1, np.int32)
    prior[:100] = np.arange(100)
    o = sl.track_frame(fr, s, perturbed(), prior)
    assert o["counts"].tolist() == [n, n, 100, n, n - 100, 0, n - 100, n]
    assert (o["reason"][:100] == strack_ref.SKIP).all() and (o["match"][:100] == -1).all() and (o["outcome"][:100] == -1).all()
    assert np.array_equal(o["match"][100:], np.arange(100, n)) and np.array_equal(o["kp_point"], np.arange(n))
    assert np.array_equal(o["edges"], np.arange(n))                     # they are edges: the same list as without a prior
    assert o["T_out"].tobytes() == tracked["T_out"].tobytes() and o["inliers"] == n
    # a prior that names OTHER points: the keypoints are taken, so their true points find nothing
    prior[:100] = np.arange(100)[::-1]
    o = sl.track_frame(fr, s, perturbed(), prior)
    assert (o["reason"][:100] == strack_ref.SKIP).all() and np.array_equal(o["kp_point"][:100], np.arange(100)[::-1])
    assert o["counts"][2] == 100 and o["counts"][6] == n - 100


def ratio_frame():
    """strack_ref.ratio_scene as a slot's arrays: every keypoint with a depth, the entry pose the identity"""
    ss, pp = strack_ref.ratio_scene(5)
    p = pp[0]
    m = len(p["kp_level"])
    fr = dict(px=p["kp_px"], level=p["kp_level"], desc=p["kp_desc"], depth=np.full(m, 4.0), has_mp=np.zeros(m, np.uint8))
    return fr, ss[0]


def test_ratio_rule_frame():
    fr, s = ratio_frame()
    o = sl.track_frame(fr, s, sl.IDENTITY)
    fired = o["outcome"] == strack_ref.RATIO
    # point i sees its own two keypoints only, 10 bits and d2 bits away, on one level: the rule fires exactly where 10 > 0.8 d2
    d2 = strack_ref.hamming_matrix(s["pt_desc"], fr["desc"])[np.arange(len(fired)), 2 * np.arange(len(fired)) + 1]
    assert np.array_equal(fired, 10.0 > 0.8 * d2) and fired.sum() >= 1 and (o["match"][fired] == -1).all()
    assert np.array_equal(o["match"][~fired], 2 * np.flatnonzero(~fired)) and (o["outcome"][~fired] == strack_ref.MATCHED).all()
    claimed = set(o["match"][o["match"] >= 0].tolist())
    assert set(np.flatnonzero(o["kp_point"] >= 0).tolist()) == claimed and o["counts"][6] == len(claimed) == o["counts"][7]
    loose = sl.track_frame(fr, s, sl.IDENTITY, ratio=1.0)
    assert (loose["outcome"] == strack_ref.RATIO).sum() == 0 and loose["counts"][6] == o["counts"][6] + fired.sum()


def test_contention_more_points_than_keypoints():
    ss, pp = strack_ref.contention_scene(3, strack_ref.LOCAL)
    p = pp[0]
    m = len(p["kp_level"])
    fr = dict(px=p["kp_px"], level=p["kp_level"], desc=p["kp_desc"], depth=np.full(m, 4.0), has_mp=np.zeros(m, np.uint8))
    o = sl.track_frame(fr, ss[0], sl.IDENTITY, th_dist=256, ratio=1e300)
    assert o["counts"][3] == 96 and o["counts"][0] == 24 and (o["outcome"] == strack_ref.NO_CANDIDATE).sum() > 20
    got = o["match"][o["match"] >= 0]
    assert len(set(got.tolist())) == len(got) == o["counts"][6] <= 24   # a keypoint is claimed once
    assert (o["kp_point"][got] == np.flatnonzero(o["match"] >= 0)).all()


def test_two_edges_keep_the_pose(scene):
    fr, s = scene
    two = {k: v[:2] for k, v in fr.items()}
    T0 = perturbed()
    o = sl.track_frame(two, {k: v[:2] for k, v in s.items()}, T0)
    assert o["counts"][6] == 2 and o["counts"][7] == 2 and o["status"] == 1 and o["T_out"].tobytes() == T0.tobytes()
    assert not o["outlier"].any() and (o["chi2"] == -1.0).all() and o["inliers"] == 0 and o["round_status"][0] == popt_ref.FAILED
    assert o["kp_point"].tolist() == [0, 1]                             # the associations are reported; they just do not reach the optimiser
    ok = sl.track_frame(two, {k: v[:2] for k, v in s.items()}, T0, min_edges=2, pose=sl.pose_params(0.1, min_edges=2))
    assert ok["status"] == 0 and (ok["chi2"] >= 0).all()


def test_empty_set_with_a_prior_of_50(scene):
    """the frame's edges are its prior: the prior has to name points, so the set here holds the 50 points and every one is skipped"""
    fr, s = scene
    n = len(fr["level"])
    small = {k: v[100:150] for k, v in s.items()}
    prior = np.full(n, -1, np.int32)
    prior[100:150] = np.arange(50)
    o = sl.track_frame(fr, small, perturbed(), prior)
    assert o["counts"].tolist() == [n, n, 50, 50, 0, 0, 0, 50] and (o["reason"] == strack_ref.SKIP).all() and o["status"] == 0
    assert np.array_equal(o["edges"], np.arange(100, 150)) and o["inliers"] == 50 and np.abs(o["T_out"] - sl.TRUTH).max() < 1e-12
    # a set of 0 points: nothing is searched, no prior can name a point, no edge
    e = sl.track_frame(fr, dict(), perturbed())
    assert e["counts"].tolist() == [n, n, 0, 0, 0, 0, 0, 0] and e["status"] == 1 and len(e["match"]) == 0 and (e["kp_point"] == -1).all()
    assert e["T_out"].tobytes() == perturbed().tobytes()


def test_joined_outputs_of_a_call(scene, tracked):
    fr, s = scene
    n = len(fr["level"])
    e = sl.track_frame(fr, dict(), perturbed())
    o = sl.joined([tracked, e, tracked], 400)
    assert o["kp_point"].shape == (3, 400) and (o["kp_point"][:, n:] == -1).all() and (o["chi2"][:, n:] == -1.0).all()
    assert not o["outlier"][:, n:].any() and o["offsets"].tolist() == [0, n, n, 2 * n] and o["match"].shape == (2 * n,)
    assert np.array_equal(o["match"][n:], tracked["match"]) and o["proj"].shape == (2 * n, 3) and o["T_out"].shape == (3, 7)
    assert sl.MAX_FRAMES == 1024 and sl.MAX_SETS == 64 and sl.MAX_PAIRS == 4194304
