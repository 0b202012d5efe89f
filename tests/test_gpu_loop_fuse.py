"""ygz::LoopClosing::FuseLoop on the MI355X, on the rendered loop scene of tests/loop_driver.py as tests/test_gpu_loop_correct.py sets it
up (ten old keyframes, a lead keyframe of another texture, a revisit run in a world drifted by s = 1.2, 4 degrees and 10 cm).  The sequence
is ComputeSim3, SearchLoopMapPoints, CorrectLoop, FuseLoop.  FuseLoop before the correction and a second FuseLoop return false and leave the
map bit-unchanged; the first returns true without touching a pose or a position; the number of good map points drops by exactly the points
replaced; no feature points to a bad point and f->_mappoint == p exactly when p->_obs[id(f)] == f; the current keyframe's covisibility weight
to the matched keyframe goes from 0 to at least the refined inlier pairs; every action lies where the keyframe's TRUE pose projects the loop
point, within the search radius plus section 12's 8.3 px; the distinctive descriptors equal tests/map_ref.c on the gathered descriptors; and
UpdateCovisibility(all, all) equals Frame::UpdateConnections() on the same state.  The program runs in a subprocess under a time limit
(tests/fuse_driver.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import map_ref as mr
from conftest import ROOT
from test_fuse_surface_build import build_program

pytestmark = pytest.mark.gpu

ALLOWANCE_PX = 8.3             # the pixel effect of the scene's Sim3 bounds (1 %, 0.25 degrees, 1 cm)
FUSE_TH = 4.0                  # LoopClosing::Option::_fuse_search_th
CURRENT_TH = 10.0              # the widest of the searches behind the current keyframe's matches (SearchByProjection)


def _R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("fuse"))
    so = build_program(d)
    out = os.path.join(d, "out.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fuse_driver.py"), so, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = dict(np.load(out))
    o = z["out"]
    assert o[0] == 1, "no loop was accepted"
    z["fused"] = z["fused"].reshape(-1, 4); z["fused_px"] = z["fused_px"].reshape(-1, 2); z["fused_pw"] = z["fused_pw"].reshape(-1, 3)
    z["dd_desc"] = z["dd_desc"].reshape(-1, 32); z["dd_got"] = z["dd_got"].reshape(-1, 32)
    print("loop %d -> %d: %d loop map points, %d matches; current keyframe: %d replaced + %d added; %d targets, %d hits: %d replaced + %d "
          "added, %d conflicts; %d descriptors, %d rows; good points %d -> %d; weight to the matched keyframe %d -> %d (loop group %d)"
          % (o[3], o[2], o[35], o[28], o[15], o[16], o[17], o[18], o[19], o[20], o[21], o[22], o[23], o[13], o[14], o[24], o[25], o[26]))
    return z


def test_refused_calls_change_nothing(run):
    o = run["out"]
    assert o[5] == 1 and o[8] == 1                      # SearchLoopMapPoints accepted the loop, CorrectLoop corrected it
    assert o[6] == 0 and o[7] == 1                      # FuseLoop before CorrectLoop: false, the map bit-unchanged
    assert o[11] == 0 and o[12] == 1                    # a second FuseLoop: false, the map bit-unchanged


def test_first_call_fuses_without_moving_anything(run):
    o = run["out"]
    assert o[9] == 1 and o[10] == 1 and o[34] == 1      # true; poses and positions bit-unchanged; the map did change
    assert o[17] >= 2 and o[18] > 0                     # the current keyframe and its neighbours were searched
    assert o[15] + o[16] > 0 and o[19] + o[20] > 0
    n1 = int(o[15] + o[16])
    fused = run["fused"]
    assert len(fused) == o[15] + o[16] + o[19] + o[20]
    assert (fused[:n1, 0] == o[3]).all()                # step 1 acts on the current keyframe, in feature order
    assert np.all(np.diff(fused[:n1, 1]) > 0)
    assert (fused[:n1, 3] >= 0).sum() == o[15] and (fused[n1:, 3] >= 0).sum() == o[19]
    rest = fused[n1:]                                   # step 3: keyframes by id, never the matched keyframe or its group
    assert np.all(np.diff(rest[:, 0]) >= 0) and (rest[:, 0] > o[4]).all()
    # a feature is acted on once, a replaced point is replaced once
    assert len(set(map(tuple, fused[:, :2].tolist()))) == len(fused)
    gone = fused[fused[:, 3] >= 0, 3]
    assert len(set(gone.tolist())) == len(gone)
    assert o[22] == len(run["dd_got"]) > 0 and o[23] > 0


def test_good_points_drop_by_the_points_replaced(run):
    o = run["out"]
    assert o[13] - o[14] == o[15] + o[19] > 0


def test_invariants_over_all_keyframes(run):
    o = run["out"]
    assert o[30] == 0                                   # no feature points to a bad map point
    assert o[31] == 0                                   # f->_mappoint == p exactly when p->_obs[id(f)] == f


def test_covisibility_crosses_the_loop(run):
    o = run["out"]
    conflicts1 = o[29] - (o[15] + o[16])                # matches of the current keyframe that step 1 skipped
    assert conflicts1 >= 0 and o[29] == o[28]
    assert o[24] == 0
    assert o[25] >= o[27] - conflicts1 > 0, (o[25], o[27], conflicts1)
    assert o[26] >= o[28] - conflicts1, (o[26], o[28], conflicts1)


def test_every_action_lies_where_the_true_pose_projects_the_loop_point(run):
    """the old world is the truth: the loop map points did not move, and revisit keyframe k's true pose is rev_T[k - lead - 1]"""
    o, K4 = run["out"], run["K4"]
    lead, n1 = int(o[4]), int(o[15] + o[16])
    worst = -np.inf
    for n, (kf, feat, L, q) in enumerate(run["fused"]):
        T = run["rev_T"][int(kf) - lead - 1]
        X = _R(T[:4]) @ run["fused_pw"][n] + T[4:]
        assert X[2] > 0
        uv = np.array([K4[0] * X[0] / X[2] + K4[2], K4[1] * X[1] / X[2] + K4[3]])
        pred = int(run["fused_pred"][n])
        assert pred >= 0
        r = (CURRENT_TH if n < n1 else FUSE_TH) * 2 ** pred
        err = np.abs(uv - run["fused_px"][n]).max()
        worst = max(worst, err - r)
        assert err < r + ALLOWANCE_PX, (n, kf, feat, L, err, r)
    print("largest excess over the radius: %.2f px (allowance %.1f)" % (worst, ALLOWANCE_PX))


def test_distinctive_descriptors_equal_the_restatement(run):
    off, desc = run["dd_offsets"], run["dd_desc"]
    assert np.all(np.diff(off) >= 2)                    # a point that gained an observation has at least two
    ref = mr.distinctive(off, desc)
    assert np.array_equal(ref["desc"], run["dd_got"])


def _records(a):
    out, i = {}, 0
    while i < len(a):
        kf, n = int(a[i]), int(a[i + 1])
        conn = a[i + 2:i + 2 + 2 * n].reshape(-1, 2)
        i += 2 + 2 * n
        m = int(a[i])
        cov = a[i + 1:i + 1 + 2 * m].reshape(-1, 2)
        i += 1 + 2 * m
        out[kf] = (conn, cov)
    return out


def test_update_covisibility_equals_update_connections(run):
    o = run["out"]
    dev, host, before = _records(run["cov_dev"]), _records(run["cov_host"]), _records(run["cov_before"])
    assert sorted(dev) == sorted(host) == sorted(run["kf_ids"].tolist())
    crossing = 0
    for kf in dev:
        (dc, dv), (hc, hv) = dev[kf], host[kf]
        assert np.array_equal(dc, hc), kf               # _connected_keyframe_weights
        assert np.array_equal(dv[:, 1], hv[:, 1]), kf   # _cov_weights, heaviest first
        assert np.all(np.diff(dv[:, 1]) <= 0)
        for w in np.unique(dv[:, 1]):                   # _cov_keyframes within groups of equal weight
            assert sorted(dv[dv[:, 1] == w, 0].tolist()) == sorted(hv[hv[:, 1] == w, 0].tolist()), (kf, w)
            if not np.array_equal(dv, before[kf][1]):             # a list this call wrote: equal weights by the smaller id (one it left
                assert np.all(np.diff(dv[dv[:, 1] == w, 0]) > 0)  # alone, a keyframe that shares nothing, keeps the scene's hand-made order)
        if kf > o[4]:
            crossing += int((dc[:, 0] < o[4]).sum())
    # only a point with two observations links keyframes, in this scene a loop map point that gained one: the keyframes that observe such
    # a point are the rows FuseLoop rewrote, and the only ones the call over all keyframes rewrites
    assert o[32] == o[23] > 0
    assert crossing > 0                                 # revisit keyframes are connected to old ones now
