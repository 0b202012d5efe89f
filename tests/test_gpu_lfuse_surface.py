"""ygz::StereoMapper::SearchInNeighbors / MapPointCulling on the MI355X, through tests/cpp/lfuse_surface.cpp in a subprocess under a time limit,
on a synthetic stereo map built from arrays as tests/test_gpu_smap_surface.py builds its own: seven keyframes -- the current one (0), three
neighbours (1, 2, 3), two second neighbours (4 behind 1, 5 behind 2) and a bad one (6, in the current keyframe's covisible list) -- that all
see 250 landmarks at 2-12 m with 0.3 px of noise, 60 % of the features with a right column, a level per landmark, descriptors that agree up
to four bits.  Every landmark is split over two or three independent duplicate MapPoints (each observed by a group of the keyframes, placed
within 5 mm of the landmark), a fifth of the features have no point, 4 % of the points are bad (their features still name them), a tenth of
the landmarks carry the descriptor of another one.

SearchInNeighbors equals the device search on the same arrays followed by the Python walk (tests/lfuse_ref.py), action for action; the point
lists and skip flags of both calls are the stated ones; afterwards no keyframe observes two good points through one feature or one good point
twice, every _obs entry points back; the number of distinct good points falls; UpdateCovisibility(GetTouched(), all) leaves the recount of
the fused map on the current keyframe, no weight below what it was and the targets' at least the shared-landmark counts; LocalBundleAdjustment accepts the fused map; a
refused device call leaves the map unchanged; MapPointCulling (a mapper without right columns, _cull_min_obs = 1) equals the Python rule on a list that exercises
its four branches and _cnt_visible = 0; CreateNewMapPoints and CreateKeyframePoints fill the recent list in creation order."""
import os
import subprocess

import numpy as np
import pytest

import lfuse_ref as lf
import smap_ref as sm
from conftest import make_ctx

pytestmark = pytest.mark.gpu
K4 = (500.0, 500.0, 320.0, 240.0)
BASELINE = 0.1
KEYFRAME, CULL_KF = 0, 5
COV = {0: [1, 6, 2, 3], 1: [0, 4, 2], 2: [5, 0, 1], 3: [1], 4: [], 5: [], 6: []}
TARGETS = [1, 4, 2, 5, 3]                                          # the interleaved walk over COV
MOVES = ([0.3, 0.0, 0.0], [0.0, 0.0, 0.3], [-0.3, 0.1, 0.0], [0.5, 0.0, 0.1], [0.1, 0.0, 0.5], [0.0, 0.3, 0.0])
NAMES = [("kf_poses", np.float64), ("kf_bad", np.uint8), ("kf_cov", np.int32), ("ft_kf", np.int32), ("ft_px", np.float64), ("ft_level", np.int32),
         ("ft_depth", np.float64), ("ft_ur", np.float64), ("ft_desc", np.uint8), ("ft_node", np.int32), ("ft_mp", np.int32), ("mp_pos", np.float64),
         ("mp_bad", np.uint8), ("cull_edit", np.int32)]


def world(seed=47):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K4
    bf = fx * BASELINE
    q0 = sm.small_quat(rng, 0.15)
    T0 = np.concatenate([q0, rng.normal(size=3) * 0.3])
    poses = [T0]
    for move in MOVES:
        dq = sm.small_quat(rng, 0.02)
        q = sm.quat_mul(dq, q0)
        poses.append(np.concatenate([q / np.linalg.norm(q), sm.quat_to_R(dq) @ (T0[4:] - np.array(move))]))
    K, P = len(poses), 250
    px0 = np.stack([rng.uniform(60, 580, P), rng.uniform(60, 420, P)], 1)
    z0 = rng.uniform(2.0, 12.0, P)
    Pc = np.stack([(px0[:, 0] - cx) / fx * z0, (px0[:, 1] - cy) / fy * z0, z0], 1)
    X = (Pc - T0[4:]) @ sm.quat_to_R(q0)
    base = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    node, level = np.arange(P) % 12, rng.integers(0, 3, P)
    for j in range(24, P, 10):
        base[j] = base[j - 12]                                   # the same node and the same descriptor as another landmark: wrong matches
    seen = [sm.project(np.asarray(T), X, K4) for T in poses]
    mp_pos, mp_bad, rows = [], [], []
    for j in range(P):
        kfs = [k for k in range(K) if 10 < seen[k][0][j, 0] < 630 and 10 < seen[k][0][j, 1] < 470 and seen[k][1][j] > 0.5]
        groups = rng.integers(0, int(rng.integers(2, 4)), len(kfs))                  # two or three duplicate points per landmark
        ids = {}
        for k, g in zip(kfs, groups):
            mp = -1
            if rng.random() >= 0.2:                              # a fifth of the features have no point
                if g not in ids:
                    ids[g] = len(mp_pos)
                    mp_pos.append(X[j] + rng.normal(size=3) * 0.005)
                    mp_bad.append(rng.random() < 0.04)
                mp = ids[g]
            u, v = seen[k][0][j] + rng.normal(size=2) * 0.3
            z = seen[k][1][j]
            stereo = rng.random() < 0.6
            ur = u - bf / z + rng.normal() * 0.2 if stereo else -1.0
            if ur < 0:
                stereo, ur = False, -1.0
            d = base[j].copy()
            for bit in rng.integers(0, 256, 4):
                d[bit // 8] ^= np.uint8(1 << (bit % 8))
            rows.append((k, u, v, int(level[j]), bf / (u - ur) if stereo else -1.0, ur, d, int(node[j]), mp, j))
    for k in range(K):
        for _ in range(20):                                       # features without a counterpart
            rows.append((k, rng.uniform(10, 630), rng.uniform(10, 470), 0, -1.0, -1.0, rng.integers(0, 256, 32, dtype=np.uint8), int(rng.integers(0, 12)), -1, -1))
    rows = [rows[i] for i in rng.permutation(len(rows))]
    cov = []
    for k in range(K):
        cov += [len(COV[k])] + COV[k]
    c = CULL_KF
    edit = [[(1, 1, 1, c), (0, 1, 5, c), (0, 1, 1, c - 2), (0, 3, 4, c - 3), (0, 1, 1, c), (0, 0, 0, c - 3)][i % 6] for i in range(4000)]
    return dict(kf_poses=np.array(poses), kf_bad=np.array([0] * 6 + [1], np.uint8), kf_cov=np.array(cov, np.int32),
                ft_kf=np.array([r[0] for r in rows], np.int32), ft_px=np.array([[r[1], r[2]] for r in rows]),
                ft_level=np.array([r[3] for r in rows], np.int32), ft_depth=np.array([r[4] for r in rows]), ft_ur=np.array([r[5] for r in rows]),
                ft_desc=np.stack([r[6] for r in rows]).astype(np.uint8), ft_node=np.array([r[7] for r in rows], np.int32),
                ft_mp=np.array([r[8] for r in rows], np.int32), mp_pos=np.array(mp_pos), mp_bad=np.array(mp_bad, np.uint8),
                cull_edit=np.array(edit, np.int32), landmark=np.array([r[9] for r in rows]))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_lfuse_surface_build import build_program
    d = str(tmp_path_factory.mktemp("lfuse_gpu"))
    exe = build_program(d)
    w = world()
    for name, t in NAMES:
        np.ascontiguousarray(w[name], t).tofile(os.path.join(d, name + ".bin"))
    r = subprocess.run([exe, "run", d, str(KEYFRAME), str(CULL_KF)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rows_of = [np.flatnonzero(w["ft_kf"] == k) for k in range(len(w["kf_poses"]))]
    start = np.concatenate([[0], np.cumsum([len(r_) for r_ in rows_of])])
    read = lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)
    return w, rows_of, start, read


def load_map(w, rows_of, start, f, s, mono=False):
    """the dumped map <s> as the dict map of tests/lfuse_ref.py (ids are the program's); mono: the mapper was given no right columns"""
    mp, obs, feat = f(s + "_mp", np.int64).reshape(-1, 6), f(s + "_mp_obs", np.int64).reshape(-1, 3), f(s + "_feat", np.int64)
    points = {int(r[0]): dict(bad=bool(r[5]), obs={}, cnt_found=int(r[4]), cnt_visible=int(r[3]), first_seen=int(r[1])) for r in mp}
    for pid, k, ix in obs:
        points[int(pid)]["obs"][int(k)] = int(ix)
    features = {k: [int(x) for x in feat[start[k]:start[k + 1]]] for k in range(len(rows_of))}
    stereo = {k: [bool(x >= 0) and not mono for x in w["ft_ur"][rows_of[k]]] for k in range(len(rows_of))}
    return lf.make_map(points, features, stereo)


def same_map(m, w, rows_of, start, f, s):
    got = load_map(w, rows_of, start, f, s)
    assert set(got["points"]) == set(m["points"])
    assert got["features"] == m["features"]
    for pid, p in got["points"].items():
        q = m["points"][pid]
        assert (p["bad"], p["obs"], p["cnt_found"], p["cnt_visible"]) == (q["bad"], q["obs"], q["cnt_found"], q["cnt_visible"]), pid


def problem_of(w, rows_of, k, skip):
    r = rows_of[k]
    return dict(T=w["kf_poses"][k], kp_px=w["ft_px"][r], kp_level=np.maximum(w["ft_level"][r], 0), kp_desc=w["ft_desc"][r],
                kp_ur=np.where(w["ft_ur"][r] >= 0, w["ft_ur"][r], -1.0), pt_skip=skip, set=0)


def good_points_of(m, kfs):
    out, seen = [], set()
    for k in kfs:
        for pid in m["features"][k]:
            if pid >= 0 and not m["points"][pid]["bad"] and pid not in seen and m["points"][pid]["obs"]:
                seen.add(pid)
                out.append(pid)
    return out


def n_good(m):
    return len({pid for fs in m["features"].values() for pid in fs if pid >= 0 and not m["points"][pid]["bad"]})


def shared(m, a, b):
    return len({p for p in m["features"][a] if p >= 0 and not m["points"][p]["bad"]} & {p for p in m["features"][b] if p >= 0 and not m["points"][p]["bad"]})


def test_search_in_neighbors_is_the_device_search_and_the_walk(out, hip_lib):
    w, rows_of, start, f = out
    m = load_map(w, rows_of, start, f, "before")
    before = lf.make_map(m["points"], m["features"], m["stereo"])
    ret = f("sin_ret", np.int32)
    assert list(f("sin_targets", np.int64)) == TARGETS and ret[1] == len(TARGETS) and ret[2] == 0
    assert any(p["bad"] for p in m["points"].values()) and any(pid >= 0 and m["points"][pid]["bad"] for fs in m["features"].values() for pid in fs)
    ctx = make_ctx(hip_lib, width=640, height=480, levels=4, max_frames=2, intrinsics=K4)
    actions, touched = [], set()
    try:
        for r, (frames, sources) in enumerate([(TARGETS, [KEYFRAME]), ([KEYFRAME], TARGETS)]):
            p = "s%d" % r
            pts = [int(x) for x in f(p + "_points", np.int64)]
            assert pts == good_points_of(m, sources) and len(pts) > 100          # the map as it is by now: the reverse set follows the forward walk
            n = len(pts)
            skip = np.array([[1 if k in m["points"][pid]["obs"] else 0 for pid in pts] for k in frames], np.uint8)
            assert np.array_equal(f(p + "_skip", np.uint8).reshape(len(frames), n), skip) and skip.any() and not skip.all()
            pw, dmax = f(p + "_pw", np.float64).reshape(n, 3), f(p + "_dmax", np.float64)
            ids = list(f("mp_ids", np.int64))
            assert np.array_equal(pw, w["mp_pos"][[ids.index(pid) for pid in pts]])
            for i in range(0, n, 7):                             # PointAttributes: |P - O_ref| 2^level of the observation with the lowest key
                k0 = min(m["points"][pts[i]]["obs"])
                T = w["kf_poses"][k0]
                centre = -sm.quat_to_R(T[:4]).T @ T[4:]
                lv = w["ft_level"][rows_of[k0][m["points"][pts[i]]["obs"][k0]]]
                assert abs(dmax[i] - np.linalg.norm(pw[i] - centre) * 2.0 ** lv) <= 1e-9 * dmax[i]
            sets = [dict(pw=pw, pt_desc=f(p + "_desc", np.uint8).reshape(n, 32), pt_dmax=dmax, pt_normal=f(p + "_normal", np.float64).reshape(n, 3))]
            pbs = [problem_of(w, rows_of, k, skip[q]) for q, k in enumerate(frames)]
            got = ctx.local_fuse_search(sets, pbs, K4, baseline=BASELINE)
            match = f(p + "_match", np.int32)
            assert np.array_equal(got["match"], match) and (match >= 0).sum() == ret[4 if r == 0 else 7] > 30
            assert np.array_equal(got["match"], lf.search(sets, pbs, np.array(K4), 640, 480, 4, baseline=BASELINE)["match"])
            hits = [(k, pts[i], int(match[q * n + i])) for q, k in enumerate(frames) for i in range(n) if match[q * n + i] >= 0]
            actions += lf.walk(m, hits, touched)
    finally:
        ctx.close()
    fus = [tuple(int(x) for x in r) for r in f("sin_fusions", np.int64).reshape(-1, 5)]
    assert fus == actions
    kinds = np.bincount([a[0] for a in actions], minlength=4)
    print("fusions: added %d, replaced into the point %d, into the feature's point %d, conflicts %d" % tuple(kinds))
    assert (kinds > 0).all()
    assert ret[0] == kinds[0] + kinds[1] + kinds[2] and ret[8] == kinds[0] and ret[9] == kinds[1] + kinds[2] and ret[10] == kinds[3]
    same_map(m, w, rows_of, start, f, "sin")
    assert list(f("sin_touched", np.int64)) == sorted(touched) and KEYFRAME in touched
    # no feature with two points, no point twice in a keyframe, every observation points back
    for pid, p in m["points"].items():
        for k, ix in p["obs"].items():
            assert m["features"][k][ix] == pid or p["bad"]
    for k, fs in m["features"].items():
        goods = [pid for pid in fs if pid >= 0 and not m["points"][pid]["bad"]]
        assert len(goods) == len(set(goods))
        for ix, pid in enumerate(fs):
            if pid >= 0 and not m["points"][pid]["bad"]:
                assert m["points"][pid]["obs"].get(k) == ix
    print("distinct good points: %d before, %d after" % (n_good(before), n_good(m)))
    assert n_good(m) < n_good(before) - 50
    # the distinctive descriptors of the current keyframe's points
    dd, mp = f("sin_mp_dd", np.uint8), f("sin_mp", np.int64).reshape(-1, 6)
    own = set(good_points_of(m, [KEYFRAME]))
    assert ret[11] == len(own) and all(dd[i] for i in range(len(mp)) if int(mp[i, 0]) in own)
    # covisibility: the recount of the fused map; nothing fell, the targets rose
    conn = {int(k): int(v) for k, v in f("sin_conn", np.int64).reshape(-1, 2)}
    for k in range(6):
        if k != KEYFRAME:
            assert conn.get(k, 0) == shared(m, KEYFRAME, k) >= shared(before, KEYFRAME, k)
    assert all(conn[k] > shared(before, KEYFRAME, k) for k in TARGETS)
    # ... to at least the shared-landmark counts: the landmarks that both keyframes saw through a feature with a good point before the call
    def landmarks(k):
        r = rows_of[k]
        has = np.array([pid >= 0 and not before["points"][pid]["bad"] for pid in before["features"][k]])
        return set(w["landmark"][r][has & (w["landmark"][r] >= 0)])
    counts = {k: len(landmarks(KEYFRAME) & landmarks(k)) for k in TARGETS}
    print("shared landmarks:", counts)
    assert all(conn[k] >= counts[k] > shared(before, KEYFRAME, k) for k in TARGETS)
    print("weights of the current keyframe:", {k: (shared(before, KEYFRAME, k), conn[k]) for k in TARGETS})
    cov = f("sin_cov", np.int64).reshape(-1, 2)
    assert set(cov[:, 0]) <= set(TARGETS) and np.all(np.diff(cov[:, 1]) <= 0) and np.all(cov[:, 1] >= 15)
    assert f("sin_ba", np.int32)[0] == 1 and f("sin_ba", np.int32)[1] > 100


def test_refused_device_call_leaves_the_map_unchanged(out):
    w, rows_of, start, f = out
    assert list(f("bad_ret", np.int32)) == [0, 0, 0]
    for k in ("feat", "mp", "mp_obs", "mp_dd"):
        assert f("bad_" + k, np.uint8).tobytes() == f("before_" + k, np.uint8).tobytes(), k


def test_culling_is_the_python_rule_and_the_recent_list_is_in_creation_order(out):
    w, rows_of, start, f = out
    n1, n2, culled, n_after, n_cleared = f("cull_ret", np.int32)
    recent = [int(x) for x in f("cull_recent", np.int64)]
    assert n1 >= 6 and n2 >= 6 and recent == [int(x) for x in f("cull_created", np.int64)] and len(recent) == n1 + n2 and n_cleared == 0
    m = load_map(w, rows_of, start, f, "edited", mono=True)       # this mapper was given no right columns: every side counts 1
    state = {pid: (m["points"][pid]["bad"], lf.n_obs(m, pid)) for pid in recent}
    keep, dead = lf.cull(m, recent, CULL_KF, min_obs=1, found_ratio=0.25)
    assert keep == [int(x) for x in f("cull_after", np.int64)] and len(dead) == culled and n_after == len(keep)
    same_map(m, w, rows_of, start, f, "cull")
    # every branch was taken: bad, found ratio, too few observations (with and without _cnt_visible = 0), survived and dropped, stays
    edit = w["cull_edit"][:len(recent)]
    gone = [pid for pid in recent if pid not in keep and pid not in dead]
    assert any(state[p][0] for p in gone) and any(not state[p][0] for p in gone)
    assert any(e[2] == 5 for p, e in zip(recent, edit) if p in dead) and any(e[2] == 0 for p, e in zip(recent, edit) if p in dead)
    assert any(e[2] == 0 for p, e in zip(recent, edit) if p in gone) and any(e[3] == CULL_KF - 2 for p, e in zip(recent, edit) if p in dead)
    assert any(e[3] == CULL_KF - 2 for p, e in zip(recent, edit) if p in keep) and any(e[3] == CULL_KF and not e[0] for p, e in zip(recent, edit) if p in keep)
