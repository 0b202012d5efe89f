"""ygz::Relocalizer on the MI355X (include/ygz/Algorithm/Relocalizer.h): a map of keyframes built through the class surfaces from a rendered
synth sequence (map points from the keyframes' depth images, a synthetic vocabulary); kidnapped frames of the same trajectory (pose reset to
identity) relocalise within bounds of the ground truth; a frame of another texture returns false and leaves its pose, features, BoW vectors
and the map as they were; a relocalised frame is tracked into the next one; the Memory form equals the explicit list.  The program runs in
a subprocess under a time limit (tests/reloc_driver.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# bounds on the relocalised pose (translation, rotation): about twice the largest error of the first MI355X run, 3.9 mm and 0.11 degrees
# (DESIGN.md section 10); the next frame, tracked from the relocalised one, keeps the starting bounds of 2 cm and 0.5 degrees
T_BOUND_M, R_BOUND_DEG = 0.008, 0.25
T_NEXT_M, R_NEXT_DEG = 0.02, 0.5


def _rot_deg(q1, q2):
    d = abs(float(np.dot(q1 / np.linalg.norm(q1), q2 / np.linalg.norm(q2))))
    return np.degrees(2 * np.arccos(min(1.0, d)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from test_reloc_surface_build import build_program
    d = tmp_path_factory.mktemp("reloc_gpu")
    so = build_program(str(d))
    out = os.path.join(str(d), "reloc.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reloc_driver.py"), so, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(out)
    print("relocalisation:", z["out"].tolist(), "wall %.3f s" % float(z["wall"]))
    return z


def test_kidnapped_frames_relocalise(run):
    o, gt = run["out"][:-1], run["gt"][:-1]
    for q in range(len(o)):
        assert o[q, 0] == 1, ("query", q, o[q, :19])
        T = o[q, 1:8]
        assert np.abs(T[4:] - gt[q, 4:]).max() < T_BOUND_M, (q, T, gt[q])
        assert _rot_deg(T[:4], gt[q, :4]) < R_BOUND_DEG, (q, T, gt[q])
        assert o[q, 11] >= 50 and o[q, 12] >= o[q, 11] and o[q, 13] >= 0 and o[q, 9] >= 1


def test_unseen_scene_returns_false_and_changes_nothing(run):
    o = run["out"][-1]
    assert o[0] == 0, o[:19]
    assert o[15] == 1 and o[16] == 1 and o[13] == -1
    assert np.array_equal(o[1:8], [0, 0, 0, 1, 0, 0, 0]) and o[12] == 0


def test_tracked_after_relocalising(run):
    o, gt = run["out"][:-1], run["gt_next"][:-1]
    for q in range(len(o)):
        Ta = o[q, 27:34]                                   # after SparseImageAlignment against the relocalised frame
        assert np.abs(Ta[4:] - gt[q, 4:]).max() < T_NEXT_M and _rot_deg(Ta[:4], gt[q, :4]) < R_NEXT_DEG, (q, Ta, gt[q])
        assert o[q, 17] >= 50 and o[q, 18] >= 50, (q, o[q, 17:19])
        T = o[q, 19:26]                                    # after OptimizeCurrentPoseOnly over the matched map points
        assert np.abs(T[4:] - gt[q, 4:]).max() < T_NEXT_M and _rot_deg(T[:4], gt[q, :4]) < R_NEXT_DEG, (q, T, gt[q])


def test_memory_form_equals_explicit_list(run):
    assert (run["out"][:, 14] == 1).all()


def test_vocabulary_score_refuses_other_scoring_types(run):
    assert float(run["refused"]) == 0.0 and float(run["same"]) == pytest.approx(1.0, abs=1e-15)
