"""ygz::StereoTracker on the MI355X, through tests/cpp/strack_surface.cpp in a subprocess under a time limit, on a synthetic stereo map built
from arrays: six keyframes around the origin (one bad) that see 400 landmarks at 2-8 m, a last frame that holds 70 % of them and a current
frame 0.15 m further along the optical axis that sees 80 %, 60 % of its keypoints with a right column, a level and an angle per landmark,
descriptors that agree up to a few bits, 100 keypoints of nothing, a few landmarks nobody observes (Matcher::PointAttributes refuses them)
and a few bad ones.

TrackWithMotionModel: the point list, levels and angles are the stated ones; the search equals the restatement on the arrays the class
uploaded (GetSearch), at the predicted pose and with the direction of the Python rule; the matched features carry the points; _cnt_found is
unchanged; features the optimiser marked bad lost their point.  LocalKeyFrames equals the Python rule.  TrackLocalMap: the local point list
is the stated one, the search equals the restatement, and _cnt_visible, _cnt_found and _track_in_view moved as the Python bookkeeping says;
_last_seen is untouched.  Without right columns the direction is 0; below _min_matches_motion the call retries with twice the window, returns
0 and leaves the predicted pose and no map point on the frame."""
import os
import subprocess

import numpy as np
import pytest

import smap_ref as sm
import strack_ref as st

pytestmark = pytest.mark.gpu
K4 = (500.0, 500.0, 320.0, 240.0)
BASELINE = 0.1
L = 4
K = 6
COV = {0: [1, 2, 5], 1: [0, 2], 2: [3, 1], 3: [5, 4], 4: [], 5: [0]}
BAD_KF = 3
NAMES = [("kf_poses", np.float64), ("kf_bad", np.uint8), ("kf_cov", np.int32), ("ft_kf", np.int32), ("ft_px", np.float64), ("ft_level", np.int32),
         ("ft_angle", np.float64), ("ft_ur", np.float64), ("ft_desc", np.uint8), ("ft_mp", np.int32), ("mp_pos", np.float64), ("mp_bad", np.uint8),
         ("velocity", np.float64), ("last_pose", np.float64)]
STATS = ["ret", "direction", "retried", "motion_points", "motion_matches", "motion_inliers", "motion_kept", "local_keyframes", "local_on_frame",
         "local_points", "local_cut", "local_searched", "local_matches", "local_inliers", "local_kept"]


def flip(rng, d, n):
    d = d.copy()
    for bit in rng.choice(256, n, replace=False):
        d[bit // 8] ^= np.uint8(1 << (bit % 8))
    return d


def world(seed=61):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K4
    bf = fx * BASELINE
    P = 400
    px0 = np.stack([rng.uniform(40, 600, P), rng.uniform(40, 440, P)], 1)
    z0 = rng.uniform(2.5, 8.0, P)
    X = np.stack([(px0[:, 0] - cx) / fx * z0, (px0[:, 1] - cy) / fy * z0, z0], 1)
    base = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    level, angle = rng.integers(0, 3, P), rng.uniform(0, 360, P)
    poses = []
    for k in range(K):
        q = sm.small_quat(rng, 0.03)
        poses.append(np.concatenate([q, rng.uniform(-0.15, 0.15, 3)]))
    last = np.concatenate([sm.small_quat(rng, 0.02), [0.02, -0.01, 0.0]])
    vq = sm.small_quat(rng, 0.01)
    velocity = np.concatenate([vq, [0.005, -0.004, -0.15]])                      # 0.15 m forward
    cur = np.concatenate([sm.quat_mul(vq, last[:4]), sm.quat_to_R(vq) @ last[4:] + velocity[4:]])
    mp_bad = (rng.random(P) < 0.03).astype(np.uint8)
    unobserved = rng.random(P) < 0.03                                           # no keyframe sees them: PointAttributes refuses
    rows = []

    def feature(k, T, j, noise, bits, mp):
        (uv,), (z,) = sm.project(np.asarray(T), X[j:j + 1], K4)
        u, v = uv + rng.normal(size=2) * noise
        ur = u - bf / z + rng.normal() * 0.2 if rng.random() < 0.6 else -1.0
        rows.append((k, u, v, int(level[j]), (angle[j] + rng.uniform(-3, 3)) % 360.0, ur if ur >= 0 else -1.0, flip(rng, base[j], bits), mp))

    def visible(T, j):
        (uv,), (z,) = sm.project(np.asarray(T), X[j:j + 1], K4)
        return z > 0.5 and 10 < uv[0] < 630 and 10 < uv[1] < 470
    for j in range(P):
        for k in range(K):
            if not unobserved[j] and rng.random() < 0.6 and visible(poses[k], j):
                feature(k, poses[k], j, 0.3, int(rng.integers(0, 5)), j if rng.random() < 0.9 else -1)
        if rng.random() < 0.7 and visible(last, j):
            feature(K, last, j, 0.3, int(rng.integers(0, 5)), j)
        if rng.random() < 0.8 and visible(cur, j):
            feature(K + 1, cur, j, 0.3, int(rng.integers(0, 8)), -1)
    for k in range(K + 2):
        for _ in range(100 if k == K + 1 else 15):                                # keypoints of nothing
            rows.append((k, rng.uniform(10, 630), rng.uniform(10, 470), int(rng.integers(0, 4)), rng.uniform(0, 360), -1.0,
                         rng.integers(0, 256, 32, dtype=np.uint8), -1))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    cov = []
    for k in range(K):
        cov += [len(COV[k])] + COV[k]
    return dict(kf_poses=np.array(poses), kf_bad=np.array([1 if k == BAD_KF else 0 for k in range(K)], np.uint8), kf_cov=np.array(cov, np.int32),
                ft_kf=np.array([r[0] for r in rows], np.int32), ft_px=np.array([[r[1], r[2]] for r in rows]), ft_level=np.array([r[3] for r in rows], np.int32),
                ft_angle=np.array([r[4] for r in rows]), ft_ur=np.array([r[5] for r in rows]), ft_desc=np.stack([r[6] for r in rows]).astype(np.uint8),
                ft_mp=np.array([r[7] for r in rows], np.int32), mp_pos=X, mp_bad=mp_bad, velocity=velocity, last_pose=last)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_strack_surface_build import build_program
    d = str(tmp_path_factory.mktemp("strack_gpu"))
    exe = build_program(d)
    w = world()
    for name, t in NAMES:
        np.ascontiguousarray(w[name], t).tofile(os.path.join(d, name + ".bin"))
    r = subprocess.run([exe, "run", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rows_of = [np.flatnonzero(w["ft_kf"] == k) for k in range(K + 2)]
    read = lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)
    ids = read("mp_ids", np.int64)
    return w, rows_of, read, ids, {int(v): i for i, v in enumerate(ids)}


def stats(read, s):
    return dict(zip(STATS, [int(x) for x in read(s + "_ret", np.int32)]))


def observed(w, rows_of):
    """per landmark: {keyframe id (= index): feature index within the keyframe}"""
    obs = {}
    for k in range(K):
        for ix, row in enumerate(rows_of[k]):
            if w["ft_mp"][row] >= 0:
                obs.setdefault(int(w["ft_mp"][row]), {})[k] = ix
    return obs


def restate(w, rows_of, read, q, mode):
    """the restatement on the arrays the class uploaded and the current frame's keypoints"""
    cur = rows_of[K + 1]
    n = len(read(q + "_points", np.int64))
    s = dict(pw=read(q + "_pw", np.float64).reshape(-1, 3), pt_desc=read(q + "_desc", np.uint8).reshape(-1, 32))
    th, direction = read(q + "_head", np.float64)
    p = dict(T=read(q + "_T", np.float64), th=float(th), mode=mode, direction=int(direction), kp_px=w["ft_px"][cur], kp_level=w["ft_level"][cur],
             kp_desc=w["ft_desc"][cur], kp_angle=w["ft_angle"][cur], set=0)
    if mode == st.FRAME:
        s.update(pt_level=read(q + "_level", np.int32), pt_angle=read(q + "_angle", np.float64))
    else:
        s.update(pt_dmax=read(q + "_dmax", np.float64), pt_normal=read(q + "_normal", np.float64).reshape(-1, 3))
        p["kp_taken"] = read(q + "_taken", np.uint8)
    return n, s, p


def same_search(read, q, want, level=True):
    for k in ("match", "dist", "reason", "outcome"):
        assert np.array_equal(read(q + "_" + k, np.int32), want[k]), (q, k)
    assert read(q + "_proj", np.float64).tobytes() == want["proj"].tobytes()
    assert np.array_equal(read(q + "_counts", np.int32), want["counts"][0])
    if level:
        assert np.array_equal(read(q + "_level", np.int32), want["level"])


def test_track_with_motion_model(out):
    w, rows_of, read, ids, index_of = out
    last, cur = rows_of[K], rows_of[K + 1]
    obs = observed(w, rows_of)
    # the point list: last's features with a good, observed point, in feature order
    want = [int(w["ft_mp"][r]) for r in last if w["ft_mp"][r] >= 0 and not w["mp_bad"][w["ft_mp"][r]] and int(w["ft_mp"][r]) in obs]
    refused = [int(w["ft_mp"][r]) for r in last if w["ft_mp"][r] >= 0 and int(w["ft_mp"][r]) not in obs]
    got = [index_of[int(v)] for v in read("s0_points", np.int64)]
    assert got == want and len(refused) > 0 and any(w["mp_bad"][w["ft_mp"][r]] for r in last if w["ft_mp"][r] >= 0)
    rows = [r for r in last if w["ft_mp"][r] >= 0 and not w["mp_bad"][w["ft_mp"][r]] and int(w["ft_mp"][r]) in obs]
    assert np.array_equal(read("s0_level", np.int32), w["ft_level"][rows]) and np.array_equal(read("s0_angle", np.float64), w["ft_angle"][rows])
    assert np.array_equal(read("s0_pw", np.float64).reshape(-1, 3), w["mp_pos"][want])
    # the predicted pose and the direction
    T = read("s0_T", np.float64)
    vq, lp = w["velocity"], w["last_pose"]
    pred = np.concatenate([sm.quat_mul(vq[:4], lp[:4]), sm.quat_to_R(vq[:4]) @ lp[4:] + vq[4:]])
    assert np.allclose(T, pred, atol=1e-12) or np.allclose(T, np.concatenate([-pred[:4], pred[4:]]), atol=1e-12)
    s = stats(read, "m")
    assert s["direction"] == st.direction(lp, T, BASELINE) == 1 and s["retried"] == 0 and read("s0_head", np.float64)[0] == 7.0
    # the search is the restatement's on what was uploaded
    n, S, P = restate(w, rows_of, read, "s0", st.FRAME)
    P["kp_ur"] = np.where(w["ft_ur"][cur] >= 0, w["ft_ur"][cur], -1.0)
    ref = st.search([S], [P], K4, 640, 480, L)
    same_search(read, "s0", ref, level=False)
    assert s["motion_points"] == n and s["motion_matches"] == ref["counts"][0, 0] >= 100 and ref["n_gated"].sum() > 0
    feat, bad = read("m_feat", np.int64), read("m_bad", np.uint8)
    m = ref["match"]
    assert len(feat) == len(cur)
    # the frame afterwards: matched features carry their point unless the optimiser marked them bad
    expect = np.full(len(cur), -1, np.int64)
    for i, j in enumerate(m):
        if j >= 0:
            expect[j] = ids[want[i]]
    expect[bad != 0] = -1
    assert np.array_equal(feat, expect) and s["ret"] == s["motion_kept"] == int((expect >= 0).sum()) >= 100 and s["motion_inliers"] >= 100
    assert (bad != 0).sum() == (m >= 0).sum() - s["ret"]
    # found points are counted in TrackLocalMap only; nothing else moved either
    mp = read("m_mp", np.int64).reshape(-1, 4)
    assert (mp[:, 0] == 1).all() and (mp[:, 1] == 1).all() and (mp[:, 2] == 0).all()
    # the optimised pose is near the true one (the prediction was exact up to the keypoint noise)
    assert np.abs(read("m_pose", np.float64)[4:] - T[4:]).max() < 0.05


def test_local_keyframes_and_track_local_map(out):
    w, rows_of, read, ids, index_of = out
    cur = rows_of[K + 1]
    obs = observed(w, rows_of)
    feat0 = read("m_feat", np.int64)
    on_frame = [index_of[int(v)] if v >= 0 else None for v in feat0]
    points = {j: dict(bad=bool(w["mp_bad"][j]), obs=obs.get(j, {})) for j in range(len(w["mp_bad"]))}
    kfs = {k: dict(bad=k == BAD_KF, cov=COV[k]) for k in range(K)}
    want_lk, want_ref = st.local_keyframes(on_frame, points, kfs)
    lk = [int(v) for v in read("lk", np.int64)]
    assert lk == want_lk and int(read("lk_ref", np.int64)[0]) == want_ref and BAD_KF not in lk and len(lk) >= 4
    # the local point list: keyframes in list order, features by index, good, observed, each once, not on the frame
    seen = set(j for j in on_frame if j is not None and not w["mp_bad"][j])
    want = []
    for k in lk:
        for r in rows_of[k]:
            j = int(w["ft_mp"][r])
            if j >= 0 and not w["mp_bad"][j] and j not in seen:
                seen.add(j)
                want.append(j)
    got = [index_of[int(v)] for v in read("s1_points", np.int64)]
    assert got == want and len(want) > 50
    taken = read("s1_taken", np.uint8)
    assert np.array_equal(taken != 0, feat0 >= 0)
    n, S, P = restate(w, rows_of, read, "s1", st.LOCAL)
    P["kp_ur"] = np.where(w["ft_ur"][cur] >= 0, w["ft_ur"][cur], -1.0)
    assert np.array_equal(P["T"], read("m_pose", np.float64)) and P["th"] == 1.0
    ref = st.search([S], [P], K4, 640, 480, L)
    same_search(read, "s1", ref)
    s = stats(read, "l")
    assert s["local_keyframes"] == len(lk) and s["local_points"] == n and s["local_cut"] == 0 and s["local_on_frame"] == int((feat0 >= 0).sum())
    assert s["local_searched"] == ref["counts"][0, 1] > 20 and s["local_matches"] == ref["counts"][0, 0] > 10
    # the frame afterwards
    feat, bad = read("l_feat", np.int64), read("l_bad", np.uint8)
    expect = feat0.copy()
    for i, j in enumerate(ref["match"]):
        if j >= 0:
            assert expect[j] < 0
            expect[j] = ids[want[i]]
    assert np.array_equal(feat, expect)
    assert s["ret"] == s["local_kept"] == int(((feat >= 0) & (bad == 0)).sum()) >= 100
    # the counters: visible, found, in view -- and _last_seen untouched
    inliers = [index_of[int(v)] for v, b in zip(feat, bad) if v >= 0 and not b]
    moves = st.track_local_bookkeeping([j for j in on_frame if j is not None], want, ref["reason"], ref["match"], inliers)
    mp0, mp = read("m_mp", np.int64).reshape(-1, 4), read("l_mp", np.int64).reshape(-1, 4)
    for j in range(len(mp)):
        dv, df, iv = moves.get(j, (0, 0, False))
        assert (mp[j, 0] - mp0[j, 0], mp[j, 1] - mp0[j, 1], bool(mp[j, 2])) == (dv, df, iv), j
    assert s["local_inliers"] == len(inliers) and np.array_equal(mp[:, 3], mp0[:, 3])
    assert sum(1 for v in moves.values() if v[0]) > s["local_on_frame"]


def test_mono_and_too_few_matches(out):
    w, rows_of, read, ids, index_of = out
    cur = rows_of[K + 1]
    s = stats(read, "mono")
    assert s["direction"] == 0 and read("mono_s0_head", np.float64)[1] == 0 and s["ret"] >= 100
    n, S, P = restate(w, rows_of, read, "mono_s0", st.FRAME)
    ref = st.search([S], [P], K4, 640, 480, L)                                   # kp_ur NULL: all mono
    same_search(read, "mono_s0", ref, level=False)
    assert ref["n_gated"].sum() == 0
    s = stats(read, "few")
    assert s["ret"] == 0 and s["retried"] == 1 and read("few_s0_head", np.float64)[0] == 14.0 and s["motion_inliers"] == 0
    n, S, P = restate(w, rows_of, read, "few_s0", st.FRAME)
    P["kp_ur"] = np.where(w["ft_ur"][cur] >= 0, w["ft_ur"][cur], -1.0)
    ref = st.search([S], [P], K4, 640, 480, L)
    same_search(read, "few_s0", ref, level=False)
    assert s["motion_matches"] == ref["counts"][0, 0] > 0
    assert (read("few_feat", np.int64) == -1).all() and np.array_equal(read("few_pose", np.float64), read("few_s0_T", np.float64))
    mp = read("few_mp", np.int64).reshape(-1, 4)
    assert (mp[:, 0] == 1).all() and (mp[:, 1] == 1).all()
