"""The definition of the stereo odometry on resident slots (tests/svo_ref.py) on exact synthetic arrays, without an
image and without a GPU: the three formulas against a second writing, the exact scene, the pose convention, and the three crafted pairs (the
retry that succeeds, too few matches, no depth).

Measured on the exact scene (300 points, depths 8 .. 20 m, the current camera 0.1 m ahead and turned by 0.21 degrees, T_init the identity):
the largest |T_rel - truth| over the seven components is 1.02e-15 (the translation's z; the quaternion is off by less than 4e-18).  The test
asserts ten times that, 1.02e-14."""
import numpy as np
import pytest

import popt_ref
import strack_ref
import svo_ref as sv

K = popt_ref.DEFAULT_K
T_REL_MEASURED = 1.02e-15
T_REL_BOUND = 10 * T_REL_MEASURED


@pytest.fixture(scope="module")
def scene():
    return sv.exact_scene()


@pytest.fixture(scope="module")
def tracked(scene):
    return sv.track_pair(*scene)


def test_formulas_against_a_second_writing():
    rng = np.random.default_rng(3)
    n = 200
    px = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1)
    depth = rng.uniform(-1, 10, n)
    depth[::17] = np.nan
    depth[5] = 0.0
    depth[6] = 1e-3                                                    # u - bf / depth far below zero: a mono keypoint
    has_mp = (rng.uniform(size=n) < 0.8).astype(np.uint8)
    has = sv.has_depth(depth, has_mp)
    fx, fy, cx, cy = K
    bf = fx * 0.1
    pw, skip = sv.unproject(px, depth, has, K)
    ur = sv.right_columns(px, depth, has, 0.1, K)
    for i in range(n):
        d = float(depth[i])
        want = bool(has_mp[i]) and (not np.isnan(d)) and d > 0
        assert bool(has[i]) == want and skip[i] == (0 if want else 1)
        if want:
            u, v = float(px[i, 0]), float(px[i, 1])
            assert pw[i, 0] == ((u - cx) / fx) * d and pw[i, 1] == ((v - cy) / fy) * d and pw[i, 2] == d
            assert ur[i] == u - bf / d
        else:
            assert (pw[i] == 0).all() and ur[i] == -1.0
    assert has[6] == bool(has_mp[6]) and (not has[6] or ur[6] < 0)
    assert not has[::17].any() and not has[5]
    # the edges: matched points in point order, kind by the sign of the right column
    match = np.full(n, -1)
    match[[3, 9, 4, 100]] = [7, 6, 0, 50]
    kp_px, kp_level = rng.uniform(0, 600, (n, 2)), rng.integers(0, 3, n).astype(np.int32)
    kp_ur = np.where(np.arange(n) % 2 == 0, rng.uniform(0, 600, n), -1.0)
    idx, X, obs, lvl, kind = sv.edges(match, pw, kp_px, kp_ur, kp_level)
    assert idx.tolist() == [3, 4, 9, 100]
    for e, (i, j) in enumerate([(3, 7), (4, 0), (9, 6), (100, 50)]):
        assert (X[e] == pw[i]).all() and obs[e].tolist() == [kp_px[j, 0], kp_px[j, 1], kp_ur[j]] and lvl[e] == kp_level[j]
        assert kind[e] == (2 if kp_ur[j] >= 0 else 1)


def test_exact_scene_tracks_every_point(scene, tracked):
    last, cur = scene
    o = tracked
    n = len(last["level"])
    assert o["status"] == 0 and o["retried"] == 0
    assert o["counts"].tolist() == [n, n, n, n, n, 0, 0, 0]
    assert np.array_equal(o["match"], np.arange(n)) and (o["dist"] == 0).all() and (o["outcome"] == strack_ref.MATCHED).all()
    assert o["inliers"] == n and not o["outlier"].any() and (o["chi2"] >= 0).all() and o["rounds_run"] == 4
    err = np.abs(o["T_rel"] - sv.TRUTH).max()
    print("max |T_rel - truth| = %.3e (measured %.3e, bound %.3e)" % (err, T_REL_MEASURED, T_REL_BOUND))
    assert err <= T_REL_BOUND


def test_pose_convention(scene, tracked):
    """T_rel takes last-camera coordinates to current-camera coordinates, and current = T_rel o last"""
    last, cur = scene
    pw, _ = sv.unproject(last["px"], last["depth"], np.ones(len(last["depth"]), bool), K)
    Pc = sv.se3_apply(tracked["T_rel"], pw)
    u, v = K[0] * (Pc[:, 0] / Pc[:, 2]) + K[2], K[1] * (Pc[:, 1] / Pc[:, 2]) + K[3]
    assert np.abs(np.stack([u, v], 1) - cur["px"]).max() < 1e-9 and np.abs(Pc[:, 2] - cur["depth"]).max() < 1e-12
    # the inverse does not: the current camera is AHEAD of the last one, so points come closer
    assert (Pc[:, 2] < pw[:, 2]).all() and tracked["T_rel"][6] < 0
    # world -> camera poses chain on the left: a world point seen by the last camera at T_lw lands in the current camera through T_rel o T_lw
    T_lw = np.concatenate([popt_ref._quat([0.2, -0.4, 0.1], 0.3), [0.5, -1.0, 2.0]])
    T_cw = sv.se3_mul(tracked["T_rel"], T_lw)
    Rl = popt_ref.w_rotation(T_lw)
    world = (pw - T_lw[4:]) @ Rl                                       # R^T (X - t)
    assert np.abs(sv.se3_apply(T_cw, world) - Pc).max() < 1e-12


def test_retry_at_twice_the_window(scene):
    last, cur = scene
    a = 0.0085                                                         # 0.97 degrees of yaw: 9 .. 12 pixels, between th and 2 th
    T0 = sv.se3_mul(np.array([0, np.sin(a), 0, np.cos(a), 0, 0, 0]), sv.TRUTH)
    first = sv.track_pair(last, cur, T_init=T0, min_matches=0)
    assert first["counts"][3] == 0 and first["counts"][7] == 0       # nothing within th
    o = sv.track_pair(last, cur, T_init=T0)
    n = len(last["level"])
    assert o["retried"] == 1 and o["counts"][7] == 1 and o["status"] == 0 and o["counts"][3] == n
    assert np.array_equal(o["match"], np.arange(n)) and o["inliers"] == n
    assert np.abs(o["T_rel"] - sv.TRUTH).max() <= T_REL_BOUND


def test_too_few_matches_fails_and_keeps_the_pose():
    last, cur = sv.exact_scene(n=12, seed=11)
    T0 = sv.TRUTH.copy()
    T0[4] += 1e-3
    o = sv.track_pair(last, cur, T_init=T0)
    assert o["counts"][3] == 12 and o["retried"] == 1 and o["status"] == 1
    assert o["T_rel"].tobytes() == T0.tobytes()
    assert o["round_status"][0] == popt_ref.FAILED and o["rounds_run"] == 1 and o["inliers"] == 0
    assert not o["outlier"].any() and (o["chi2"] == -1.0).all() and len(o["edges"]) == 0
    assert (o["match"] >= 0).sum() == 12                               # the matches are reported; they just do not reach the optimiser


def test_last_frame_without_any_depth(scene):
    last, cur = scene
    blind = dict(last, has_mp=np.zeros(len(last["level"]), np.uint8))
    o = sv.track_pair(blind, cur)
    n = len(last["level"])
    assert o["counts"].tolist() == [n, 0, n, 0, 0, 0, 0, 1] and o["status"] == 1
    assert (o["reason"] == strack_ref.SKIP).all() and (o["match"] == -1).all() and (o["outcome"] == -1).all()
    assert o["T_rel"].tobytes() == sv.IDENTITY.tobytes() and o["round_status"][0] == popt_ref.FAILED
    nodepth = dict(last, depth=np.full(n, np.nan))
    assert sv.track_pair(nodepth, cur)["counts"].tolist() == [n, 0, n, 0, 0, 0, 0, 1]


def test_padding_of_a_call(scene, tracked):
    o = sv.padded([tracked, tracked], 400)
    n = len(scene[0]["level"])
    assert o["match"].shape == (2, 400) and (o["match"][:, n:] == -1).all() and (o["chi2"][:, n:] == -1.0).all() and not o["outlier"][:, n:].any()
    assert (o["proj"][:, n:] == 0).all() and np.array_equal(o["match"][1, :n], tracked["match"]) and o["T_rel"].shape == (2, 7)
