"""ygz::BundleAdjuster on the MI355X: LocalBundleAdjustment on a synthetic stereo map (8 keyframes on a ring, 80 points seen four times, half
the observations with a right column, 10 % gross outliers) equals the C call on the exported problem and the restatement; the fixed
keyframes keep their bits; the outlier observations are gone on both sides and nothing else in the map has changed; _erase_outliers false
erases nothing; GlobalBundleAdjustment equals the C call; a FAILED call leaves the map bit-unchanged; without SetURight every edge is mono.
The program tests/cpp/sba_surface.cpp runs in a subprocess under a time limit."""
import os
import subprocess

import numpy as np
import pytest

import gba_ref as gb
import sba_ref as sb

pytestmark = pytest.mark.gpu
KEYFRAME, COV = 4, (3, 5)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_sba_surface_build import build_program
    d = str(tmp_path_factory.mktemp("sba_gpu"))
    exe = build_program(d)
    g = sb.scene(8, 80, 4, outliers=0.1, seed=21)
    behind = np.array(g["points"]).copy()
    l = int(g["edge_point"][np.flatnonzero(g["edge_pose"] == KEYFRAME)[0]])
    T = g["poses"][KEYFRAME]
    behind[l] = 1.5 * (-gb.rotation(T[:4]).T @ T[4:])
    for name, a, t in [("kf_poses", g["poses"], np.float64), ("points", g["points"], np.float64), ("points_behind", behind, np.float64),
                       ("ob_kf", g["edge_pose"], np.int32), ("ob_point", g["edge_point"], np.int32), ("ob_level", g["level"], np.int32),
                       ("ob_px", g["obs"], np.float64), ("ob_kind", g["kind"], np.uint8)]:
        np.ascontiguousarray(a, t).tofile(os.path.join(d, name + ".bin"))
    r = subprocess.run([exe, "run", d, str(KEYFRAME), ",".join(map(str, COV))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return g, l, (lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype))


def _problem(f, s):
    return dict(poses=f(s + "_poses", np.float64).reshape(-1, 7), fixed=f(s + "_fixed", np.uint8), points=f(s + "_points", np.float64).reshape(-1, 3),
                edge_pose=f(s + "_edge_pose", np.int32), edge_point=f(s + "_edge_point", np.int32), obs=f(s + "_obs", np.float64).reshape(-1, 3),
                kind=f(s + "_kind", np.uint8), level=f(s + "_level", np.int32), K=tuple(f("camera", np.float64)), baseline=0.1)


def _map(f, s):
    return dict((k, f(s + "_" + k, t).tobytes()) for k, t in [("poses", np.float64), ("points", np.float64), ("feat", np.int64), ("obs", np.int64),
                                                               ("rest", np.uint8)])


def test_local_equals_the_c_call_and_the_restatement(out):
    g, _, f = out
    assert tuple(f("camera", np.float64)) == sb.K4
    pb = _problem(f, "local")
    ret, n_out, rounds_run, left_out = f("local_ret", np.int32)
    want = sb.optimize(pb)
    assert ret == 1 and rounds_run == want["rounds_run"] == 2 and n_out == int(want["outlier"].sum()) > 0
    for k, t in [("poses_out", np.float64), ("points_out", np.float64), ("chi2", np.float64), ("outlier", np.uint8)]:
        key = k.replace("_out", "")
        assert f("local_" + k, t).tobytes() == f("local_abi_" + k, t).tobytes() == np.ascontiguousarray(want[key], t).tobytes(), k
    assert np.array_equal(f("local_status", np.int32), want["status"]) and np.array_equal(f("local_abi_status", np.int32), want["status"])
    assert np.array_equal(f("local_inliers", np.int32), want["inliers"])
    # the composition: free are the keyframe and its covisible ones, every other keyframe that sees one of their points is fixed
    ids = f("local_kf_ids", np.int64)
    free = set((KEYFRAME,) + COV)
    assert list(pb["fixed"]) == [0 if k in free else 1 for k in ids] and set(ids) > free
    pts_of_free = sorted(set(g["edge_point"][np.isin(g["edge_pose"], list(free))]))
    assert len(f("local_point_ids", np.int64)) == len(pts_of_free) - left_out and left_out == 0
    assert (pb["kind"] == 2).sum() > 0 and (pb["kind"] == 1).sum() > 0


def test_fixed_keyframes_keep_their_bits_and_the_rest_is_rewritten(out):
    g, _, f = out
    ids, fixed = f("local_kf_ids", np.int64), f("local_fixed", np.uint8)
    before, after = f("before_poses", np.float64).reshape(-1, 7), f("local_map_poses", np.float64).reshape(-1, 7)
    po = f("local_poses_out", np.float64).reshape(-1, 7)
    for v, k in enumerate(ids):
        if fixed[v]:
            assert after[k].tobytes() == before[k].tobytes() == po[v].tobytes()
        else:
            assert np.abs(after[k] - po[v]).max() < 1e-12 and after[k].tobytes() != before[k].tobytes()      # through SE3: a rotation matrix in between
    pid = f("local_point_ids", np.int64)
    pa, pb_ = f("local_map_points", np.float64).reshape(-1, 3), f("before_points", np.float64).reshape(-1, 3)
    xo = f("local_points_out", np.float64).reshape(-1, 3)
    assert pa[pid].tobytes() == xo.tobytes()
    rest = np.setdiff1d(np.arange(len(pa)), pid)
    assert pa[rest].tobytes() == pb_[rest].tobytes()


def test_outlier_observations_are_gone_on_both_sides_and_nothing_else_changed(out):
    g, _, f = out
    outlier = f("local_outlier", np.uint8).astype(bool)
    ids, pid = f("local_kf_ids", np.int64), f("local_point_ids", np.int64)
    ep, el, ef = f("local_edge_pose", np.int32), f("local_edge_point", np.int32), f("local_edge_feature", np.int32)
    gone = set((int(pid[el[e]]), int(ids[ep[e]]), int(ef[e])) for e in np.flatnonzero(outlier))
    obs_b = set(map(tuple, f("before_obs", np.int64).reshape(-1, 3)))
    obs_a = set(map(tuple, f("local_map_obs", np.int64).reshape(-1, 3)))
    assert gone and gone <= obs_b and obs_a == obs_b - gone
    fb, fa = f("before_feat", np.int64), f("local_map_feat", np.int64)
    counts = np.bincount(g["edge_pose"], minlength=8)
    start = np.concatenate([[0], np.cumsum(counts)])
    changed = set((int(k), int(i)) for k in range(8) for i in range(counts[k]) if fa[start[k] + i] != fb[start[k] + i])
    assert changed == set((k, i) for _, k, i in gone) and all(fa[start[k] + i] == -1 for k, i in changed)
    assert f("local_map_rest", np.uint8).tobytes() == f("before_rest", np.uint8).tobytes()
    assert outlier[f("local_kind", np.uint8) != 0].sum() == len(gone)


def test_erase_outliers_false_erases_nothing(out):
    _, _, f = out
    a, b, c = _map(f, "noerase_map"), _map(f, "before"), _map(f, "local_map")
    assert a["feat"] == b["feat"] and a["obs"] == b["obs"] and a["rest"] == b["rest"]
    assert a["poses"] == c["poses"] and a["points"] == c["points"]
    assert f("noerase_outlier", np.uint8).tobytes() == f("local_outlier", np.uint8).tobytes() and f("noerase_ret", np.int32)[1] > 0


def test_global_equals_the_c_call_and_the_restatement(out):
    _, _, f = out
    pb = _problem(f, "global")
    want = sb.optimize(pb, rounds=1, robust_rounds=1, iterations=(10,))
    assert list(f("global_ret", np.int32)[:3]) == [1, int(want["outlier"].sum()), 1]
    assert list(pb["fixed"]) == [1] + [0] * 7 and list(f("global_kf_ids", np.int64)) == list(range(8))
    for k, t in [("poses_out", np.float64), ("points_out", np.float64), ("chi2", np.float64), ("outlier", np.uint8)]:
        assert f("global_" + k, t).tobytes() == f("global_abi_" + k, t).tobytes() == np.ascontiguousarray(want[k.replace("_out", "")], t).tobytes(), k
    a, b = _map(f, "global_map"), _map(f, "before")
    assert a["feat"] == b["feat"] and a["obs"] == b["obs"] and a["rest"] == b["rest"]                       # no observation is erased
    pid = f("global_point_ids", np.int64)
    assert sorted(pid) == list(range(80)) and a["poses"] != b["poses"]
    assert f("global_map_points", np.float64).reshape(-1, 3)[pid].tobytes() == f("global_points_out", np.float64).tobytes()


def test_failed_call_leaves_the_map_bit_unchanged(out):
    _, l, f = out
    ret, n_out, rounds_run, _ = f("failed_ret", np.int32)
    assert ret == 0 and rounds_run == 1 and f("failed_status", np.int32)[0] == sb.FAILED and n_out > 0
    assert _map(f, "failed_map") == _map(f, "before_behind")
    want = sb.optimize(_problem(f, "failed"))
    assert want["status"][0] == sb.FAILED and np.array_equal(f("failed_outlier", np.uint8), want["outlier"])


def test_without_set_uright_every_edge_is_mono(out):
    _, _, f = out
    pb = _problem(f, "mono")
    assert f("mono_ret", np.int32)[0] == 1 and np.all(pb["kind"] == 1) and np.all(pb["obs"][:, 2] == 0.0)
    want = sb.optimize(pb)
    assert f("mono_poses_out", np.float64).tobytes() == want["poses"].tobytes() and f("mono_points_out", np.float64).tobytes() == want["points"].tobytes()
    assert f("mono_points_out", np.float64).tobytes() != f("local_points_out", np.float64).tobytes()
