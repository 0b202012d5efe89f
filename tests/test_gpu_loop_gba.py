"""ygz::LoopClosing::GlobalBundleAdjustment on the MI355X, on the rendered loop scene of tests/loop_driver.py as tests/test_gpu_loop_fuse.py
sets it up, after ComputeSim3, SearchLoopMapPoints, CorrectLoop and FuseLoop.  In that scene every map point is born with one observation, so
only the fused loop map points carry two or more: the call over every keyframe in Memory (the lead keyframe and the old keyframes outside the
loop share nothing) returns false and leaves the map bit-unchanged; the call over the keyframes that observe such a point returns true, the
fixed keyframe keeps its bits, every rewritten pose and point equals tests/gba_ref.c on the exported problem bit for bit, nothing but _TCW and
_pos_world changed, the points left out and the keyframes not given are untouched, the robust cost fell, and so did the mean reprojection
error of the cross-loop observations (LoopClosing::GetFusedPairs).  The program runs in a subprocess under a time limit
(tests/gba_driver.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gba_ref as gb
from conftest import ROOT
from test_gba_surface_build import build_program

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gba"))
    so = build_program(d)
    out = os.path.join(d, "out.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gba_driver.py"), so, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = dict(np.load(out))
    o = z["out"]
    assert o[0] == 1, "no loop was accepted"
    for k, w in [("ba_poses", 7), ("ba_poses_out", 7), ("ba_points", 3), ("ba_points_out", 3), ("ba_obs", 2), ("kf_before", 7), ("kf_after", 7),
                 ("pt_before", 3), ("pt_after", 3), ("fused", 3), ("fused_px", 2)]:
        z[k] = z[k].reshape(-1, w)
    print("loop %d -> %d: %d of %d keyframes given; %d poses, %d points, %d observations, %d points left out; cost %.6g -> %.6g, status %d, "
          "%d LM iterations, %d solves, %d CG iterations (%d capped), lambda %.3g"
          % (o[3], o[2], o[27], o[33], o[15], o[16], o[17], o[18], o[24], o[25], o[19], o[20], o[21], o[22], o[23], o[26]))
    return z


@pytest.fixture(scope="module")
def replay(run):
    """the restatement on the problem the class handed over"""
    g = dict(poses=run["ba_poses"], fixed=run["ba_fixed"], points=run["ba_points"], edge_pose=run["ba_edge_pose"], edge_point=run["ba_edge_point"],
             obs=run["ba_obs"], K=tuple(run["ba_K4"]), huber=float(run["ba_huber"][0]))
    return g, gb.optimize(g)


def test_earlier_stages_succeeded(run):
    o = run["out"]
    assert o[5] == 1 and o[8] == 1 and o[9] == 1        # SearchLoopMapPoints, CorrectLoop, FuseLoop
    assert len(run["fused"]) > 0


def test_a_free_keyframe_without_an_edge_refuses_the_call(run):
    o = run["out"]
    assert o[34] == o[33] > o[27]                       # the Memory form gathered every keyframe, more than share a point
    assert o[10] == 0 and o[11] == 1                    # false, the map bit-unchanged


def test_call_returns_true_and_changes_only_poses_and_positions(run):
    o = run["out"]
    assert o[12] == 1
    assert o[13] == 1 and o[14] == 1                    # observation maps, bad flags, covisibility and the rest bit-unchanged; the geometry moved
    assert o[15] == o[27] == len(run["ba_kf_ids"]) and o[16] == len(run["ba_point_ids"]) and o[17] == len(run["ba_obs"])
    assert float(run["ba_huber"][0]) == 5.991 and o[20] >= 1 and o[20] <= 10


def test_problem_follows_the_rules(run):
    ids, fixed = run["ba_kf_ids"], run["ba_fixed"]
    assert np.all(np.diff(ids) > 0) and fixed[0] == 1 and not fixed[1:].any()
    assert len(set(run["ba_point_ids"].tolist())) == len(run["ba_point_ids"])
    assert np.all(np.diff(run["ba_edge_point"]) >= 0)                   # a point's edges are together, points in the order they were met
    assert np.bincount(run["ba_edge_point"]).min() >= 2
    for l in np.unique(run["ba_edge_point"]):                           # _obs key order: ascending keyframe id within a point
        assert np.all(np.diff(run["ba_edge_pose"][run["ba_edge_point"] == l]) > 0)
    row = {int(k): i for i, k in enumerate(run["kf_ids"])}
    assert np.array_equal(_bits(run["ba_poses"]), _bits(run["kf_before"][[row[int(k)] for k in ids]]))
    prow = {int(k): i for i, k in enumerate(run["pt_ids"])}
    assert np.array_equal(_bits(run["ba_points"]), _bits(run["pt_before"][[prow[int(k)] for k in run["ba_point_ids"]]]))
    # every cross-loop observation is an edge of the problem
    edges = set(zip(ids[run["ba_edge_pose"]].tolist(), run["ba_point_ids"][run["ba_edge_point"]].tolist()))
    assert all((int(kf), int(L)) in edges for kf, _, L in run["fused"])


def test_result_equals_the_restatement_bit_for_bit(run, replay):
    o = run["out"]
    g, ref = replay
    assert np.array_equal(_bits(run["ba_poses_out"]), _bits(ref["poses"])) and np.array_equal(_bits(run["ba_points_out"]), _bits(ref["points"]))
    assert (o[19], o[20], o[21], o[22], o[23]) == (ref["status"], ref["lm_iterations"], ref["n_solves"], ref["cg_iterations_total"], ref["cg_capped"])
    assert _bits([o[24], o[25], o[26]]).tolist() == _bits([ref["cost_initial"], ref["cost_final"], ref["lambda_"]]).tolist()
    # the map holds the solver's answer: free poses and included points rewritten, the fixed keyframe and everything else bit-unchanged
    row = {int(k): i for i, k in enumerate(run["kf_ids"])}
    want = run["kf_before"].copy()
    for i, k in enumerate(run["ba_kf_ids"]):
        if not run["ba_fixed"][i]:
            want[row[int(k)]] = ref["poses"][i]
    assert np.array_equal(_bits(run["kf_after"]), _bits(want))
    assert np.array_equal(_bits(run["kf_after"][row[int(run["ba_kf_ids"][0])]]), _bits(run["kf_before"][row[int(run["ba_kf_ids"][0])]]))
    prow = {int(k): i for i, k in enumerate(run["pt_ids"])}
    wantp = run["pt_before"].copy()
    wantp[[prow[int(k)] for k in run["ba_point_ids"]]] = ref["points"]
    assert np.array_equal(_bits(run["pt_after"]), _bits(wantp))
    assert o[18] > 0 and len(run["pt_ids"]) > len(run["ba_point_ids"])  # points were left out, and the line above shows them untouched


def test_robust_cost_fell(run, replay):
    o = run["out"]
    assert o[19] != gb.FAILED and o[25] < o[24]


def test_cross_loop_reprojection_error_fell(run):
    K = run["ba_K4"]
    row = {int(k): i for i, k in enumerate(run["kf_ids"])}
    prow = {int(k): i for i, k in enumerate(run["pt_ids"])}

    def mean_error(T, X):
        e = []
        for (kf, _, L), px in zip(run["fused"], run["fused_px"]):
            t = T[row[int(kf)]]
            P = gb.rotation(t[:4]) @ X[prow[int(L)]] + t[4:]
            e.append(np.hypot(K[0] * P[0] / P[2] + K[2] - px[0], K[1] * P[1] / P[2] + K[3] - px[1]))
        return float(np.mean(e))
    before, after = mean_error(run["kf_before"], run["pt_before"]), mean_error(run["kf_after"], run["pt_after"])
    print("mean reprojection error of the %d cross-loop observations: %.3f -> %.3f px" % (len(run["fused"]), before, after))
    assert after < before
