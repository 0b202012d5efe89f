"""CPU witnesses of tests/init_ref.c, the restatement of the reference's monocular Initializer (src/Algorithm/Initializer.cpp) that the
device path (ygz_hip_initialize) is held against: the cv::RNG sample sets, the one-sided Jacobi SVD against numpy, DecomposeE / the 8
Faugeras solutions against a noise-free ground truth, Sophus' quaternion-from-matrix against scipy, and the decisions on the two scenes of
the reference's test/test_initializer.cpp:9-45,56-59 (tests/golden/init_reference_scenes.npz)."""
import os

import numpy as np
import pytest

import init_ref as ir
from conftest import ROOT


def _ref_scene(which):
    g = np.load(os.path.join(ROOT, "tests", "golden", "init_reference_scenes.npz"))
    P = g["landmarks_" + which]
    return ir.project(g["K4"], P), ir.project(g["K4"], P + g["t2"]), g["K4"]


@pytest.mark.parametrize("n", [8, 9, 50, 3072])
def test_sample_sets_are_eight_distinct_indices_in_range(n):
    s = ir.sample_sets(n, 200)
    assert s.shape == (200, 8) and s.min() >= 0 and s.max() < n
    assert all(len(set(r)) == 8 for r in s.tolist())
    assert np.array_equal(s, ir.sample_sets(n, 200))            # a fresh cv::RNG per call: the sets depend on n alone
    assert not np.array_equal(s[0], s[1])


def test_rng_first_draws():
    """cv::RNG() state 0xffffffff: next() = (uint32)state * 4164903690 + (state >> 32); uniform(0, n) = next() % n"""
    st, out = 0xffffffff, []
    avail = list(range(100))
    for j in range(8):
        st = (st & 0xffffffff) * 4164903690 + (st >> 32)
        st &= (1 << 64) - 1
        r = (st & 0xffffffff) % len(avail)
        out.append(avail[r]); avail[r] = avail[-1]; avail.pop()
    assert ir.sample_sets(100, 1)[0].tolist() == out


@pytest.mark.parametrize("shape", [(16, 9), (8, 9), (4, 4)])
def test_null_vector_matches_numpy(shape):
    rng = np.random.default_rng(sum(shape))
    for _ in range(20):
        A = rng.normal(size=shape) * rng.uniform(0.1, 300, size=(1, shape[1]))
        if shape[0] >= shape[1]:
            A[:, -1] = A[:, :-1] @ rng.normal(size=shape[1] - 1)          # exact null space up to rounding
        x = ir.null_vector(A)
        v = np.linalg.svd(A)[2][-1]
        assert min(np.abs(x - v).max(), np.abs(x + v).max()) < 1e-10


def test_svd3_is_an_svd():
    rng = np.random.default_rng(3)
    for _ in range(50):
        A = rng.normal(size=(3, 3))
        U, s, V = ir.svd3(A)
        assert np.allclose(U @ np.diag(s) @ V.T, A, atol=1e-12)
        assert np.allclose(U.T @ U, np.eye(3), atol=1e-12) and np.allclose(V.T @ V, np.eye(3), atol=1e-12)
        assert s[0] >= s[1] >= s[2] >= 0 and np.allclose(s, np.linalg.svd(A)[1], rtol=1e-12)
        assert abs(np.linalg.det(U) - 1) < 1e-12


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def test_decompose_e_contains_the_ground_truth():
    for seed in range(10):
        rng = np.random.default_rng(seed)
        R = ir.rot(rng.normal(size=3), rng.uniform(1, 20))
        t = rng.normal(size=3); t /= np.linalg.norm(t)
        E = _skew(t) @ R * rng.uniform(0.5, 3)
        R1, R2, tt = ir.decompose_e(E)
        assert any(np.abs(Rc - R).max() < 1e-9 for Rc in (R1, R2))
        assert min(np.abs(tt - t).max(), np.abs(tt + t).max()) < 1e-9


def test_h_solutions_contain_the_ground_truth():
    K4 = ir.K4_DEFAULT
    K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])
    for seed in range(10):
        rng = np.random.default_rng(100 + seed)
        R = ir.rot(rng.normal(size=3), rng.uniform(2, 15))
        t = rng.normal(size=3) * 0.4
        nrm = np.array([0.1, -0.2, 1.0]); nrm /= np.linalg.norm(nrm); d = 3.0       # plane n^T X = d in camera 1
        H = K @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(K)
        ok, Rs, ts = ir.h_solutions(H, K4)
        assert ok
        tn = t / np.linalg.norm(t)
        assert any(np.abs(Rs[i] - R).max() < 1e-6 and np.abs(ts[i] - tn).max() < 1e-6 for i in range(8))


def test_quaternion_from_matrix_round_trips_scipy():
    Rot = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(7)
    mats = [ir.rot(rng.normal(size=3), a) for a in (0.5, 30, 100, 179, 180)] + [np.eye(3), np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])]
    for R in mats:
        q = ir.quat_from_matrix(R)
        assert abs(np.linalg.norm(q) - 1) < 1e-12
        assert np.allclose(Rot.from_quat(q).as_matrix(), R, atol=1e-12)
        qs = Rot.from_matrix(R).as_quat()
        assert min(np.abs(q - qs).max(), np.abs(q + qs).max()) < 1e-12


def test_reference_scene_planar():
    """12 coplanar landmarks at z = 2, camera 2 moved by (1, 0, 0): both models fit every point; H is scored in one direction, F in two,
    so rh = 1/3 and F is chosen, and no F solution holds 0.9 of the inliers -> TryInitialize returns false"""
    px1, px2, K4 = _ref_scene("H")
    r = ir.initialize(px1, px2, K4)["result"]
    assert r["model"] == 2 and abs(r["rh"] - 1 / 3) < 1e-6 and r["n_inliers"] == 12
    assert not r["success"] and r["n_good"] < int(0.9 * 12)
    assert np.array_equal(r["R21"], np.eye(3).ravel()) and np.array_equal(r["t21"], np.zeros(3))


def test_reference_scene_three_planes():
    """12 landmarks on z = 2, 3, 4: F, success, R21 = I, t21 parallel to (1, 0, 0), all 12 points triangulated"""
    px1, px2, K4 = _ref_scene("F")
    o = ir.initialize(px1, px2, K4)
    r = o["result"]
    assert r["success"] and r["model"] == 2 and r["n_triangulated"] == 12 and o["triangulated"].all()
    assert np.abs(r["R21"].reshape(3, 3) - np.eye(3)).max() < 1e-9
    assert np.abs(r["t21"] - np.array([1.0, 0, 0])).max() < 1e-9
    g = np.load(os.path.join(ROOT, "tests", "golden", "init_reference_scenes.npz"))
    assert np.allclose(o["pts3d"], g["landmarks_F"], atol=1e-6)          # |t| = 1 is the true baseline here


def test_reconstruct_h_on_a_plane():
    """ReconstructH itself (the fused path rarely chooses H): from the best homography of a planar scene (2 degrees of rotation, a
    sideways baseline) the accepted solution is the true motion.  (With 3-6 degrees the second-best of the 8 solutions keeps more than
    0.75 of the best one's points on this plane and ReconstructH declines, as the reference's rule says.)"""
    s = ir.scene(400, 31, planar=True, R=ir.rot([0.3, 1, 0.2], 2.0), t=np.array([0.8, 0.1, 0.0]))
    h = ir.hypotheses(s["px1"], s["px2"], ir.sample_sets(400, 200))
    o = ir.reconstruct(s["px1"], s["px2"], s["K4"], 1, h["result"]["H21"], h["inliers_h"])["result"]
    assert o["success"] and 0 <= o["solution"] < 8 and o["second_good"] < 0.75 * o["n_good"]
    R = o["R21"].reshape(3, 3)
    assert np.degrees(np.arccos(np.clip((np.trace(R.T @ s["R"]) - 1) / 2, -1, 1))) < 1.0
    assert np.degrees(np.arccos(np.clip(o["t21"] @ s["t"] / np.linalg.norm(s["t"]), -1, 1))) < 5.0


def test_model_choice_on_general_scenes_is_f():
    """what the scoring implies: F is scored in both directions, H in one, so where F fits rh stays well below 0.4"""
    for seed in (1, 2, 3):
        s = ir.scene(600, seed)
        r = ir.hypotheses(s["px1"], s["px2"], ir.sample_sets(600, 200))["result"]
        assert r["model"] == 2 and r["rh"] < 0.2


def test_degenerate_inputs_fail_definitely():
    same = np.tile([[320.0, 240.0]], (20, 1))
    r = ir.initialize(same, same, ir.K4_DEFAULT)["result"]
    assert not r["success"] and r["model"] == 0 and r["best_h"] == -1 and r["best_f"] == -1
    s = ir.scene(100, 5)
    r = ir.initialize(s["px1"], s["px1"], ir.K4_DEFAULT)["result"]
    assert not r["success"]
