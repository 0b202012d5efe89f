"""ygz::LoopClosing::CorrectLoop on the MI355X, on the rendered loop scene of tests/loop_driver.py: ten old keyframes, a lead keyframe of
another texture, a revisit run in a world drifted by s = 1.2, 4 degrees and 10 cm; the old world is the truth.  After the ComputeSim3 that
accepts the loop, CorrectLoop returns true; the matched keyframe is bit-unchanged and the other old keyframes stay where they were; the lead
keyframe is left out; the pose graph the class gathered gives the same S_out through tests/pgo_ref.c bit for bit; every revisit keyframe and
every moved point lands within what the scene's bounds on the accepted Sim3 allow of its true place; reprojections into the reference keyframe
do not change; a second call returns false and changes nothing.  The program runs in a subprocess under a time limit
(tests/correct_driver.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pgo_ref as pg
from conftest import ROOT
from test_correct_surface_build import build_program

pytestmark = pytest.mark.gpu

# the loop scene's bounds on the accepted Sim3 (tests/test_gpu_loop_closing.py): scale 1 %, rotation 0.25 degrees, translation 1 cm per axis
S_BOUND, R_BOUND_DEG, T_BOUND_M = 0.01, 0.25, 0.01
SLACK = 1e-9                   # what the optimiser may move a vertex whose edges are already satisfied


def _R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _rot_deg(Ra, Rb):
    c = (np.trace(Ra @ Rb.T) - 1) / 2
    return np.degrees(np.arccos(np.clip(c, -1, 1)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("correct"))
    so = build_program(d)
    out = os.path.join(d, "out.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "correct_driver.py"), so, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = dict(np.load(out))
    o = z["out"]
    assert o[0] == 1, "no loop was accepted"
    z["poses_before"] = z["poses_before"].reshape(-1, 7); z["poses_after"] = z["poses_after"].reshape(-1, 7)
    z["pt_before"] = z["pt_before"].reshape(-1, 3); z["pt_after"] = z["pt_after"].reshape(-1, 3); z["pt_px"] = z["pt_px"].reshape(-1, 2)
    for k in ["g_S", "g_S_out", "g_M"]:
        z[k] = z[k].reshape(-1, 8)
    z["g_edges"] = z["g_edges"].reshape(-1, 2)
    return z


def test_correct_loop_returns_true_once(run):
    o = run["out"]
    assert o[23] == 0                                   # before any accepted loop
    assert o[4] == 1 and o[7] == 1                      # corrected; nothing but poses and point positions changed
    assert o[5] == 0 and o[6] == 1                      # the second call: false, the map bit-unchanged
    n_old, cur, matched, lead = len(run["old_T"]), int(o[3]), int(o[2]), int(o[8])
    assert matched < n_old and lead == n_old and cur > lead
    print("loop %d -> %d: %d vertices, %d tree + %d covisibility + %d loop edges, %d left out, %d points moved; solver status %d, %d LM "
          "iterations, %d solves, %d CG iterations, cost %.3g -> %.3g" % (cur, matched, o[9], o[10], o[11], o[12], o[14], o[13], o[15], o[16], o[17],
                                                                          o[18], o[20], o[21]))
    assert o[9] == len(run["g_ids"]) and o[10] + o[11] + o[12] == len(run["g_edges"]) and o[12] == 1
    assert o[11] >= 1                                   # the revisit run's weight-100 pairs
    assert o[15] != pg.FAILED


def test_old_keyframes_stay_and_the_lead_is_left_out(run):
    o = run["out"]
    ids, before, after = run["kf_ids"], run["poses_before"], run["poses_after"]
    n_old, matched, lead = len(run["old_T"]), int(o[2]), int(o[8])
    m = int(np.flatnonzero(ids == matched)[0])
    assert np.array_equal(before[m].view(np.uint64), after[m].view(np.uint64))
    old = ids < n_old
    moved = np.abs(after[old] - before[old]).max()
    print("old keyframes moved by at most %.3g" % moved)
    assert moved < SLACK
    assert list(run["left_out"]) == [lead] and lead not in run["g_ids"]
    k = int(np.flatnonzero(ids == lead)[0])
    assert np.array_equal(before[k].view(np.uint64), after[k].view(np.uint64))
    pl = run["pt_kf"] == lead
    assert pl.any() and np.array_equal(run["pt_before"][pl].view(np.uint64), run["pt_after"][pl].view(np.uint64))
    # points of old keyframes do not move: those of the matched keyframe bit for bit, the others with their keyframes
    pm = run["pt_kf"] == matched
    assert pm.any() and np.array_equal(run["pt_before"][pm].view(np.uint64), run["pt_after"][pm].view(np.uint64))
    po = run["pt_kf"] < n_old
    assert np.abs(run["pt_after"][po] - run["pt_before"][po]).max() < 10 * SLACK


def test_the_gathered_graph_through_the_restatement(run):
    """the documented rules, rebuilt here from the map before the correction, give the graph the class handed over; tests/pgo_ref.c gives the
    same S_out on it bit for bit"""
    o = run["out"]
    g = dict(S=run["g_S"], fixed=run["g_fixed"], edges=run["g_edges"], M=run["g_M"])
    ref = pg.optimize(g)
    assert np.array_equal(ref["S"].view(np.uint64), run["g_S_out"].view(np.uint64))
    assert (ref["status"], ref["lm_iterations"], ref["n_solves"], ref["cg_iterations_total"], ref["cg_capped"]) == tuple(int(v) for v in o[15:20])
    assert (ref["cost_initial"], ref["cost_final"], ref["lambda_"]) == (o[20], o[21], o[22])
    ids, gid = run["kf_ids"], run["g_ids"]
    assert np.all(np.diff(gid) > 0)
    cur, matched, lead = int(o[3]), int(o[2]), int(o[8])
    assert [int(gid[v]) for v in np.flatnonzero(run["g_fixed"])] == [matched]
    # the estimate: the current keyframe is S_cw, the old ones Sim3(T_iw)
    pose = {int(i): p for i, p in zip(ids, run["poses_before"])}
    for v, i in enumerate(gid):
        if i == cur:
            assert np.array_equal(run["g_S"][v], run["S_cw"])
        elif i < lead:
            assert np.array_equal(run["g_S"][v], np.append(pose[int(i)], 1.0))
    # the edges: a tree edge per keyframe with a smaller neighbour (old run: the one before, weight 80; revisit run: the one before, weight
    # 120), the revisit run's weight-100 pairs two apart, the loop edge last
    n_old = len(run["old_T"])
    rev = [int(i) for i in gid if i > lead]
    want = [(i, i - 1) for i in range(1, n_old)] + [(i, i - 1) for i in rev[1:]] + [(i, i - 2) for i in rev[2:]] + [(cur, matched)]
    got = [(int(gid[a]), int(gid[b])) for a, b in run["g_edges"]]
    assert got == want, (got, want)


def _bounds(T_c, T_ic):
    """the rotation (degrees) and translation (metres) by which a revisit keyframe's corrected pose may miss its true one: S_i = Sim3(T_ic) o
    S_cw has S_cw's rotation error; its translation t_i' / s' misses t_i = R_ic t_c + t_ic by R_ic (t_c' / s' - t_c) + t_ic (s_d / s' - 1), and
    with |s' / s_d - 1| < e, |t_c' - s_d t_c| < sqrt(3) dt that is at most sqrt(3) dt / (s_d (1 - e)) + e / (1 - e) (|t_c| + |t_ic|)"""
    s_d = 1.2
    es = S_BOUND / (1 - S_BOUND)
    return R_BOUND_DEG, np.sqrt(3) * T_BOUND_M / (s_d * (1 - S_BOUND)) + es * (np.linalg.norm(T_c[4:]) + np.linalg.norm(T_ic)) + SLACK


def test_revisit_keyframes_land_on_their_true_poses(run):
    o = run["out"]
    ids, after, before, rev_T = run["kf_ids"], run["poses_after"], run["poses_before"], run["rev_T"]
    lead, cur = int(o[8]), int(o[3])
    T_c = rev_T[cur - lead - 1]
    checked = 0
    for k, i in enumerate(ids):
        if i <= lead or i not in run["g_ids"]:
            continue
        T = rev_T[int(i) - lead - 1]
        R_ic = _R(T[:4]) @ _R(T_c[:4]).T
        a_deg, b = _bounds(T_c, T[4:] - R_ic @ T_c[4:])
        r_err, t_err = _rot_deg(_R(after[k][:4]), _R(T[:4])), np.linalg.norm(after[k][4:] - T[4:])
        r_unc, t_unc = _rot_deg(_R(before[k][:4]), _R(T[:4])), np.linalg.norm(before[k][4:] - T[4:])
        print("keyframe %d: %.4f deg, %.5f m from the truth (allowance %.2f deg, %.5f m; uncorrected %.3f deg, %.4f m)"
              % (i, r_err, t_err, a_deg, b, r_unc, t_unc))
        assert a_deg < r_unc / 5 and b < t_unc / 5        # the check cannot pass on an uncorrected map
        assert r_err < a_deg and t_err < b
        checked += 1
    assert checked >= 3


def test_moved_points_keep_their_pixel_and_land_on_the_truth(run):
    o = run["out"]
    K4, ids, after, before = run["K4"], run["kf_ids"], run["poses_after"], run["poses_before"]
    lead, cur = int(o[8]), int(o[3])
    D = run["drift"]
    Rd, td, sd = _R(D[:4]), D[4:7], D[7]
    T_c = run["rev_T"][cur - lead - 1]
    moved = np.any(run["pt_before"] != run["pt_after"], axis=1)
    assert moved.sum() <= o[13]                         # a point recomputed to the same bits is counted as moved by the class
    moved &= run["pt_kf"] > lead                        # an old keyframe may move in its last bits, and its points with it: checked above
    assert moved.any()
    worst_px = worst_ratio = 0.0
    for i in np.unique(run["pt_kf"][moved]):
        k = int(np.flatnonzero(ids == i)[0])
        sel = moved & (run["pt_kf"] == i)
        assert sel.sum() == (run["pt_kf"] == i).sum()                  # every point of a corrected keyframe moved
        P0, P1 = run["pt_before"][sel], run["pt_after"][sel]
        Y0, Y1 = P0 @ _R(before[k][:4]).T + before[k][4:], P1 @ _R(after[k][:4]).T + after[k][4:]
        uv = lambda Y: np.stack([K4[0] * Y[:, 0] / Y[:, 2] + K4[2], K4[1] * Y[:, 1] / Y[:, 2] + K4[3]], 1)
        worst_px = max(worst_px, np.abs(uv(Y0) - uv(Y1)).max())
        # the truth: D^-1 of the old position.  P' = R_r'^T (Y0 - t_r') / s' against R_r^T (Y0 / s_d - t_r): the rotation error a turns
        # |Y0| / s' + |t_r| + b, the scale error stretches |Y0| / s_d by e / (1 - e), the translation error adds b
        truth = ((P0 - td) @ Rd) / sd
        T = run["rev_T"][int(i) - lead - 1]
        R_ic = _R(T[:4]) @ _R(T_c[:4]).T
        a_deg, b = _bounds(T_c, T[4:] - R_ic @ T_c[4:])
        es = S_BOUND / (1 - S_BOUND)
        Xc = np.linalg.norm(Y0, axis=1) / sd
        allow = np.deg2rad(a_deg) * ((1 + es) * Xc + np.linalg.norm(T[4:]) + b) + es * Xc + b
        err, unc = np.linalg.norm(P1 - truth, axis=1), np.linalg.norm(P0 - truth, axis=1)
        worst_ratio = max(worst_ratio, (err / allow).max())
        assert np.all(allow < unc / 5), (allow.max(), unc.min())
        assert np.all(err < allow), (i, err.max(), allow.min())
    print("moved points: reprojection changed by at most %.3g px; largest error / allowance %.3f" % (worst_px, worst_ratio))
    assert worst_px < 1e-6
