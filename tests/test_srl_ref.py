"""The definition of the stereo relocalisation on resident slots (tests/srl_ref.py) on exact synthetic arrays, without
an image and without a GPU: srk_ref.exact_scene (300 world points 8 .. 20 m in front of the keyframe, keyframe and frame keypoints their exact
projections with exact depths, each pair sharing a random descriptor, tests/bow_cases.ragged_vocabulary() at levelsup 1) with the frame at
TRUTH and no entry pose.

The bound on |T_opt - TRUTH|: the observations are exact to an ulp of a pixel coordinate below 640, 1.1e-13 pixels; a pixel is 20 m / 520 =
0.04 m at the far end of the scene, so an observation pins the translation to 4e-15 m and the rotation to less; 1e-12 leaves two and a half
decades for the conditioning of the 6 x 6 system.  The test prints what it measures before it asserts."""
import numpy as np
import pytest

import bow_cases as bc
import pnp_ref
import popt_ref
import srk_ref as sk
import srl_ref as rl

K = popt_ref.DEFAULT_K
T_BOUND = 1e-12


@pytest.fixture(scope="module")
def vocab():
    return sk.oracle().vocab_parse(bc.ragged_vocabulary())


@pytest.fixture(scope="module")
def scene():
    """slot 0 the keyframe, 1 the frame, 2 a keyframe with the same keypoints and unrelated descriptors; set 0 the true points, 1 each point
    moved on its own by up to two metres, 2 the first 100 points true and the rest moved"""
    kfr, fr, s = sk.exact_scene(300, 3)
    rng = np.random.default_rng(12)
    other = dict(kfr, desc=rng.integers(0, 256, kfr["desc"].shape, dtype=np.uint8))
    moved = dict(pw=s["pw"] + rng.uniform(-2.0, 2.0, s["pw"].shape))
    partly = dict(pw=np.where(np.arange(300)[:, None] < 100, s["pw"], moved["pw"]))
    frames = {0: kfr, 1: fr, 2: other}
    return frames, [s, moved, partly]


def call(scene, vocab, kf_slot, kf_set, candidates, slots=(1,), **kw):
    frames, sets = scene
    rows = np.tile(np.arange(300, dtype=np.int32), (len(kf_slot), 1))
    return rl.relocalize(frames, sets, kf_slot, kf_set, rows, list(slots), candidates, vocab, 300, K=K, **dict(dict(levelsup=1), **kw))


def test_the_true_keyframe_recovers_the_truth_and_wins(scene, vocab):
    o = call(scene, vocab, [0], [0], [[0]])
    err = np.abs(o["T_opt"][0] - sk.TRUTH).max()
    print("associations %d, PnP inliers %d, final inliers %d, |T_pnp - truth| %.3g, |T_opt - truth| %.3g"
          % (o["counts"][0, 7], o["counts"][0, 8], o["counts"][0, 9], np.abs(o["T_pnp"][0] - sk.TRUTH).max(), err))
    assert o["status"][0] == rl.RELOCALISED and o["best"][0] == 0 and o["T_out"][0].tobytes() == o["T_opt"][0].tobytes()
    assert o["counts"][0, 7] > 250 and o["counts"][0, 8] == o["counts"][0, 7] == o["counts"][0, 9] and not o["outlier"].any()
    assert err < T_BOUND
    assert np.array_equal(o["sets"][0], pnp_ref.sample_sets(int(o["counts"][0, 7]), 300))
    # prior = kp_point on this scene, and every associated keypoint names its own point
    assert np.array_equal(o["prior"], o["kp_point"]) and (o["kp_point"][0][o["kp_point"][0] >= 0] == np.flatnonzero(o["kp_point"][0] >= 0)).all()
    assert (o["pnp_inlier"][0] == (o["kp_point"][0] >= 0)).all() and ((o["chi2"][0] >= 0) == (o["kp_point"][0] >= 0)).all()


def test_unrelated_descriptors_give_status_1(scene, vocab):
    o = call(scene, vocab, [2], [0], [[0]])
    assert o["status"][0] == rl.TOO_FEW_MATCHES and o["counts"][0, 7] < 15 and o["best"][0] == -1
    for k in ("T_out", "T_pnp", "T_opt"):
        assert o[k][0].tobytes() == rl.IDENTITY.tobytes()
    assert o["pnp_success"][0] == 0 and o["pnp_n_hypotheses"][0] == 0 and o["pnp_best_sample"][0] == -1 and o["counts"][0, 8] == 0
    assert not o["pnp_inlier"].any() and (o["prior"] == -1).all() and not o["outlier"].any() and (o["chi2"] == -1.0).all() and not o["sets"].any()
    assert o["inliers"][0] == 0


def test_a_displaced_set_gives_status_2_or_3(scene, vocab):
    o = call(scene, vocab, [0, 0], [1, 2], [[0, 1]], min_final_inliers=120)
    assert o["status"].tolist() == [rl.PNP_FAILED, rl.TOO_FEW_INLIERS] and o["best"][0] == -1 and o["T_out"][0].tobytes() == rl.IDENTITY.tobytes()
    # status 2: the best hypothesis is returned as it is, nothing is optimised
    assert o["pnp_success"][0] == 0 and 3 <= o["pnp_n_inliers"][0] < 10 and o["T_opt"][0].tobytes() == o["T_pnp"][0].tobytes()
    assert o["pnp_inlier"][0].sum() == o["pnp_n_inliers"][0] and not o["outlier"][0].any() and (o["chi2"][0] == -1.0).all() and o["inliers"][0] == 0
    assert ((o["prior"][0] >= 0) == (o["pnp_inlier"][0] != 0)).all()
    # status 3: the PnP finds the true points, at most 100, the optimiser keeps them, fewer than the 120 asked for; the pose is the truth all the same
    assert o["pnp_success"][1] == 1 and 50 <= o["inliers"][1] <= o["pnp_n_inliers"][1] <= 100
    assert np.abs(o["T_opt"][1] - sk.TRUTH).max() < 1e-9 and (np.flatnonzero(o["prior"][1] >= 0) < 100).all()
    assert ((o["chi2"][1] >= 0) == (o["pnp_inlier"][1] != 0)).all() and o["inliers"][1] == (o["prior"][1] >= 0).sum()


def test_best_honours_the_callers_order(scene, vocab):
    """two candidates succeed: the first in the caller's order wins, whichever has more inliers; a failing one in front is passed over"""
    frames, sets = scene
    half = np.arange(300, dtype=np.int32)
    half[150:] = -1                                                      # the true keyframe with half its points
    rows = np.stack([np.arange(300, dtype=np.int32), half, np.arange(300, dtype=np.int32)])
    run = lambda cands: rl.relocalize(frames, sets, [0, 0, 2], [0, 0, 0], rows, [1, 1], cands, vocab, 300, K=K, levelsup=1)
    o = run([[1, 0], [2, 0, 1]])
    assert o["status"].tolist() == [0, 0, 1, 0, 0] and o["best"].tolist() == [0, 3]
    assert o["counts"][0, 9] < o["counts"][1, 9] and o["T_out"][0].tobytes() == o["T_opt"][0].tobytes() != o["T_opt"][1].tobytes()
    assert o["T_out"][1].tobytes() == o["T_opt"][3].tobytes() == o["T_opt"][1].tobytes()
    o = run([[0, 1], []])
    assert o["best"].tolist() == [0, -1] and o["T_out"][1].tobytes() == rl.IDENTITY.tobytes()
