"""ygz::StereoMapper on the MI355X, through tests/cpp/smap_surface.cpp in a subprocess under a time limit, on a synthetic stereo map: five
keyframes (the current one, neighbours moved 0.3 m sideways, 0.3 m forward and 0.3 m the other way, and one 0.05 m away, which ORB-SLAM2's
stereo rule skips), 250 points at 2-12 m seen by all of them with 0.3 px of noise, 60 % of the features with a right column and a depth,
random levels 0-2, 15 % of the features with a map point already and 5 % with a bad one (free, and detached from it when they get a new one), descriptors that agree up to four bits per observation, a tenth of the
points with the descriptor of another point (wrong matches), and features without a counterpart ("arrays"); and on a rendered rectified pair
sequence ("rendered"): five stereo keyframes of ygz_slam_amd/synth.py's textured plane, 3.5 m away, at the same five places, each pair taken
through InitFrame, FeatureDetector, StereoMatcher::ComputeStereoMatches (Feature::_depth, u_right; -1 where unmatched) and Frame::ComputeBoW
with a synthetic vocabulary by the program itself, which writes out what those calls left in the frames.

CreateKeyframePoints makes exactly the restatement's selection with the stated fields; CreateNewMapPoints over the three neighbours equals
the restatement applied to the same matcher output followed by the stated walk; a feature never ends with two points; a refused device call
leaves the map unchanged; BundleAdjuster::LocalBundleAdjustment accepts the grown map and flags exactly the edges the restatement's sba_ref
flags on the same problem."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import sba_ref as sb
import smap_ref as sm
from ygz_slam_amd import synth

pytestmark = pytest.mark.gpu
K4 = (500.0, 500.0, 320.0, 240.0)                              # of the "arrays" map; the rendered one has the configuration's default camera
BASELINE = 0.1
KEYFRAME, COV = 0, (1, 2, 3, 4)


def world(seed=31):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K4
    bf = fx * BASELINE
    q0 = sm.small_quat(rng, 0.15)
    T0 = np.concatenate([q0, rng.normal(size=3) * 0.3])
    poses = [T0]
    for move in ([0.3, 0.0, 0.0], [0.0, 0.0, 0.3], [-0.3, 0.1, 0.0], [0.05, 0.0, 0.0]):
        dq = sm.small_quat(rng, 0.02)
        q = sm.quat_mul(dq, q0)
        poses.append(np.concatenate([q / np.linalg.norm(q), sm.quat_to_R(dq) @ (T0[4:] - np.array(move))]))
    P = 250
    px0 = np.stack([rng.uniform(60, 580, P), rng.uniform(60, 420, P)], 1)
    z0 = rng.uniform(2.0, 12.0, P)
    Pc = np.stack([(px0[:, 0] - cx) / fx * z0, (px0[:, 1] - cy) / fy * z0, z0], 1)
    X = (Pc - T0[4:]) @ sm.quat_to_R(q0)
    base = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    node = np.arange(P) % 12
    for j in range(24, P, 10):
        base[j] = base[j - 12]                                   # the same node and the same descriptor as another point: wrong matches
    rows = []
    for k, T in enumerate(poses):
        px, z = sm.project(np.asarray(T), X, K4)
        for j in range(P):
            if not (10 < px[j, 0] < 630 and 10 < px[j, 1] < 470 and z[j] > 0.5):
                continue
            u, v = px[j] + rng.normal(size=2) * 0.3
            stereo = rng.random() < 0.6
            ur = u - bf / z[j] + rng.normal() * 0.2 if stereo else -1.0
            if ur < 0:
                stereo, ur = False, -1.0
            d = base[j].copy()
            for bit in rng.integers(0, 256, 4):
                d[bit // 8] ^= np.uint8(1 << (bit % 8))
            rows.append((k, u, v, int(rng.integers(0, 3)), bf / (u - ur) if stereo else -1.0, ur, d, int(node[j]), int(rng.choice([0, 1, 2], p=[0.8, 0.15, 0.05])), j))
        for _ in range(20):                                       # features without a counterpart
            rows.append((k, rng.uniform(10, 630), rng.uniform(10, 470), 0, -1.0, -1.0, rng.integers(0, 256, 32, dtype=np.uint8), int(rng.integers(0, 12)), 0, -1))
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    w = dict(kf_poses=np.array(poses), ft_kf=np.array([r[0] for r in rows], np.int32), ft_px=np.array([[r[1], r[2]] for r in rows]),
             ft_level=np.array([r[3] for r in rows], np.int32), ft_depth=np.array([r[4] for r in rows]), ft_ur=np.array([r[5] for r in rows]),
             ft_desc=np.stack([r[6] for r in rows]).astype(np.uint8), ft_node=np.array([r[7] for r in rows], np.int32),
             ft_has=np.array([r[8] for r in rows], np.uint8), point=np.array([r[9] for r in rows]))
    return w


MOVES = ([0.3, 0.0, 0.0], [0.0, 0.0, 0.3], [-0.3, 0.1, 0.0], [0.05, 0.0, 0.0])


def rendered_pairs(seed=17):
    """(poses [5, 7], left [5, 480, 640], right [5, 480, 640]): the plane Z = 2 seen from 3.5 m, the right camera 0.1 m along the left one's x axis"""
    rng = np.random.default_rng(seed)
    tex, margin = synth.make_texture(3, 640, 480, margin=420)
    c0 = np.array([0.02, -0.01, synth.PLANE_Z - 3.5])
    poses, left, right = [], [], []
    for k, move in enumerate(([0.0, 0.0, 0.0],) + MOVES):
        q = sm.small_quat(rng, 0.04)
        R = sm.quat_to_R(q)
        c = c0 + R.T @ np.array(move)
        T = np.concatenate([q, -R @ c])
        Tr = np.concatenate([q, T[4:] - np.array([BASELINE, 0.0, 0.0])])
        poses.append(T)
        left.append(synth.render(tex, margin, T, 640, 480, 1.0, 700 + k)[0])
        right.append(synth.render(tex, margin, Tr, 640, 480, 1.0, 800 + k)[0])
    return np.array(poses), np.stack(left), np.stack(right)


@pytest.fixture(scope="module", params=["arrays", "rendered"])
def out(request, tmp_path_factory):
    from test_smap_surface_build import build_program
    d = str(tmp_path_factory.mktemp("smap_gpu_" + request.param))
    exe = build_program(d)
    names = [("kf_poses", np.float64), ("ft_kf", np.int32), ("ft_px", np.float64), ("ft_level", np.int32), ("ft_depth", np.float64),
             ("ft_ur", np.float64), ("ft_desc", np.uint8), ("ft_node", np.int32), ("ft_has", np.uint8)]
    read = lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)
    if request.param == "arrays":
        w = world()
        for name, t in names:
            np.ascontiguousarray(w[name], t).tofile(os.path.join(d, name + ".bin"))
        mode = "run"
    else:
        poses, left, right = rendered_pairs()
        poses.tofile(os.path.join(d, "kf_poses.bin"))
        left.tofile(os.path.join(d, "seq_left.bin"))
        right.tofile(os.path.join(d, "seq_right.bin"))
        with open(os.path.join(d, "vocab.bin"), "wb") as fh:
            fh.write(fixtures.synthetic_vocabulary(k=6, L=2, seed=5, stop_frac=0.0))
        mode = "seq"
    r = subprocess.run([exe, mode, d, str(KEYFRAME), ",".join(map(str, COV))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    if mode == "seq":                                             # what the detector, the stereo matcher and ComputeBoW left in the frames
        w = dict((name, read(name, t)) for name, t in names)
        w["kf_poses"], w["ft_px"] = w["kf_poses"].reshape(-1, 7), w["ft_px"].reshape(-1, 2)
    # the features of keyframe k, in file order: rows of the input
    rows_of = [np.flatnonzero(w["ft_kf"] == k) for k in range(len(w["kf_poses"]))]
    start = np.concatenate([[0], np.cumsum([len(r_) for r_ in rows_of])])
    w["K"], w["rendered"] = tuple(read("camera", np.float64)), mode == "seq"
    return w, rows_of, start, read


def _map(f, s):
    return dict((k, f(s + "_" + k, t).tobytes()) for k, t in [("feat", np.int64), ("fdepth", np.float64), ("fbad", np.uint8), ("mp", np.int64),
                                                               ("mp_pos", np.float64), ("mp_obs", np.int64)])


def test_keyframe_points_are_the_restatements_selection(out):
    w, rows_of, start, f = out
    K = w["K"]
    assert K == (K4 if not w["rendered"] else (synth.FX, synth.FY, synth.CX, synth.CY))
    rows = rows_of[KEYFRAME]
    want = sm.keyframe_points(w["kf_poses"][KEYFRAME], w["ft_px"][rows], w["ft_depth"][rows], w["ft_has"][rows] == 1, K)
    sel = np.flatnonzero(want["selected"])
    ret, n_created = f("kp_ret", np.int32)
    print("keyframe: %d features, %d with a depth, %d close, %d selected" % (len(rows), want["n_depth"], want["n_close"], len(sel)))
    assert ret == n_created == len(sel) > 50 and want["n_depth"] > want["n_close"] > 0
    if w["rendered"]:                                             # the stereo matcher's leftovers are in the input
        assert (w["ft_depth"][rows] == -1).any() and want["n_depth"] > max(want["n_close"], 100) + 1 and want["n_depth"] - 1 > (want["rank"] >= 0).sum() - 1
    fb, fa = f("before_feat", np.int64), f("kp_feat", np.int64)
    n_old = int((w["ft_has"] > 0).sum())
    mp = f("kp_mp", np.int64).reshape(-1, 6)
    pos = f("kp_mp_pos", np.float64).reshape(-1, 3)
    obs = f("kp_mp_obs", np.int64).reshape(-1, 3)
    assert len(mp) == n_old + len(sel) and f("before_mp", np.int64).tobytes() == mp[:n_old].tobytes()
    new = mp[n_old:]
    # in feature order, each selected feature points at its own new point; nothing else changed
    changed = np.flatnonzero(fa != fb)
    was_bad = w["ft_has"][rows][sel] == 2                          # a selected feature either had no point or a bad one
    assert np.array_equal(changed, start[KEYFRAME] + sel) and np.all((fb[changed] == -1) != was_bad)
    assert w["rendered"] or was_bad.any()
    assert len(set(map(tuple, obs[:, 1:]))) == len(obs)             # no feature is left in a bad point's observations beside its new one
    assert np.array_equal(fa[changed], new[:, 0]) and len(set(new[:, 0])) == len(sel) and not set(new[:, 0]) & set(mp[:n_old, 0])
    kf_id = KEYFRAME                                              # the keyframes are registered in order: id = index
    assert np.all(new[:, 1] == kf_id) and np.all(new[:, 2] == kf_id) and np.all(new[:, 3] == 1) and np.all(new[:, 4] == 1) and np.all(new[:, 5] == 0)
    assert pos[n_old:].tobytes() == np.ascontiguousarray(want["pos_world"][sel]).tobytes()
    new_obs = obs[np.isin(obs[:, 0], new[:, 0])]
    assert np.array_equal(new_obs, np.stack([new[:, 0], np.full(len(sel), kf_id), sel], 1))
    assert f("kp_fdepth", np.float64).tobytes() == f("before_fdepth", np.float64).tobytes() and not f("kp_fbad", np.uint8).any()


def _problems(w, rows_of, f):
    pairs, nb_of, nb_ids = f("np_pairs", np.int32).reshape(-1, 2), f("np_pair_nb", np.int32), f("np_nb_ids", np.int64)
    pbs = []
    for q, kid in enumerate(nb_ids):
        m = pairs[nb_of == q]
        r1, r2 = rows_of[KEYFRAME][m[:, 0]], rows_of[kid][m[:, 1]]
        pbs.append(sm.normalise(dict(T1=w["kf_poses"][KEYFRAME], T2=w["kf_poses"][kid], px1=w["ft_px"][r1], px2=w["ft_px"][r2], ur1=w["ft_ur"][r1],
                                     ur2=w["ft_ur"][r2], depth1=w["ft_depth"][r1], depth2=w["ft_depth"][r2], level1=w["ft_level"][r1],
                                     level2=w["ft_level"][r2])))
    return pairs, nb_of, nb_ids, pbs


def test_new_map_points_equal_the_restatement_and_the_walk(out):
    w, rows_of, start, f = out
    pairs, nb_of, nb_ids, pbs = _problems(w, rows_of, f)
    assert list(nb_ids) == [1, 2, 3]                              # keyframe 4 is closer than the baseline
    assert np.all(np.diff(nb_of) >= 0) and len(pairs) > (60 if w["rendered"] else 200)
    has = w["ft_has"] == 1
    for q, kid in enumerate(nb_ids):                              # pairs of which a feature has a point were dropped
        m = pairs[nb_of == q]
        assert not has[rows_of[KEYFRAME][m[:, 0]]].any() and not has[rows_of[kid][m[:, 1]]].any()
    res = [sm.create(pb, w["K"]) for pb in pbs]
    code, method, X = np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res]), np.concatenate([r[2] for r in res])
    assert np.array_equal(f("np_codes", np.int32), code) and np.array_equal(f("np_methods", np.int32), method)
    print('codes', np.bincount(code, minlength=9), 'methods of the points', np.bincount(method[code == 0], minlength=4))
    assert len(np.unique(code)) >= (2 if w["rendered"] else 3) and {1, 2} <= set(np.unique(method[code == 0]))
    # the walk: neighbour order, then pair order; a feature takes at most one point
    taken, made = set(), []
    for i in np.flatnonzero(code == 0):
        a, b = (KEYFRAME, int(pairs[i, 0])), (int(nb_ids[nb_of[i]]), int(pairs[i, 1]))
        if a in taken or b in taken:
            continue
        taken |= {a, b}
        made.append(i)
    ret, n_created = f("np_ret", np.int32)
    assert ret == n_created == len(made) > (20 if w["rendered"] else 60) and len(made) < int((code == 0).sum())      # the walk's rule was needed
    n_old = int((w["ft_has"] > 0).sum())
    mp, pos = f("np_mp", np.int64).reshape(-1, 6), f("np_mp_pos", np.float64).reshape(-1, 3)
    obs = f("np_mp_obs", np.int64).reshape(-1, 3)
    new = mp[n_old:]
    assert len(new) == len(made) and np.array_equal(new[:, 0], f("np_created", np.int64)) and f("before_mp", np.int64).tobytes() == mp[:n_old].tobytes()
    assert pos[n_old:].tobytes() == np.ascontiguousarray(X[made]).tobytes()
    assert np.all(new[:, 1] == KEYFRAME) and np.all(new[:, 2] == KEYFRAME) and np.all(new[:, 3] == 2) and np.all(new[:, 4] == 2) and np.all(new[:, 5] == 0)
    fb, fa = f("before_feat", np.int64), f("np_feat", np.int64)
    db, da = f("before_fdepth", np.float64), f("np_fdepth", np.float64)
    want_feat, want_obs = fb.copy(), []
    n_was_bad = 0
    for pid, i in zip(new[:, 0], made):
        kid = int(nb_ids[nb_of[i]])
        sides = [(KEYFRAME, int(pairs[i, 0])), (kid, int(pairs[i, 1]))]
        for k, ix in sides:
            g = start[k] + ix
            n_was_bad += int(w["ft_has"][rows_of[k][ix]] == 2)
            want_feat[g] = pid
            T = w["kf_poses"][k]
            z = (sm.quat_to_R(T[:4]) @ X[i] + T[4:])[2]
            if w["ft_ur"][rows_of[k][ix]] < 0:
                assert abs(da[g] - z) <= 1e-9 * z                 # a mono side gets the point's depth in its camera
            else:
                assert da[g] == db[g]
        want_obs += [(pid, k, ix) for k, ix in sorted(sides)]
    assert np.array_equal(fa, want_feat) and (w["rendered"] or n_was_bad > 0)      # features of bad points took part and were re-pointed
    untouched = fa == fb
    assert da[untouched].tobytes() == db[untouched].tobytes() and not f("np_fbad", np.uint8).any()
    new_obs = obs[np.isin(obs[:, 0], new[:, 0])]
    assert np.array_equal(new_obs, np.array(want_obs, np.int64))
    # a feature never ends with two points
    assert len(set(map(tuple, obs[:, 1:]))) == len(obs)


def test_refused_device_call_leaves_the_map_unchanged(out):
    _, _, _, f = out
    assert list(f("bad_ret", np.int32)) == [0, 0, 0, 0, 0]
    assert _map(f, "bad") == _map(f, "before")


def test_local_bundle_adjustment_accepts_the_grown_map(out):
    w, rows_of, start, f = out
    ret, n_out, rounds_run, left_out = f("ba_ret", np.int32)
    pb = dict(poses=f("ba_poses", np.float64).reshape(-1, 7), fixed=f("ba_fixed", np.uint8), points=f("ba_points", np.float64).reshape(-1, 3),
              edge_pose=f("ba_edge_pose", np.int32), edge_point=f("ba_edge_point", np.int32), obs=f("ba_obs", np.float64).reshape(-1, 3),
              kind=f("ba_kind", np.uint8), level=f("ba_level", np.int32), K=w["K"], baseline=BASELINE)
    want = sb.optimize(pb)
    assert ret == 1 and rounds_run == want["rounds_run"] == 2
    created = f("np_created", np.int64)
    assert set(f("ba_point_ids", np.int64)) == set(created) and len(pb["edge_pose"]) == 2 * len(created)      # the new points, two edges each
    assert np.array_equal(f("ba_outlier", np.uint8), want["outlier"]) and n_out == int(want["outlier"].sum())
    assert np.array_equal(f("ba_status", np.int32), want["status"])
    kept = 1.0 - f("ba_outlier", np.uint8).mean()
    assert kept >= 1.0 - want["outlier"].mean()
    assert (pb["kind"] == 2).any() and (pb["kind"] == 1).any()
