"""ygz::StereoOdometry on the MI355X, through tests/cpp/svo_surface.cpp in a subprocess under a time limit, on three QVGA frames of a
sequence whose pictures move by 3 pixels per frame (tests/stereo_ref.py's texture), lattice keypoints that move with them, 70 % with the
scene's constant depth.

TrackPairs over (1, 0), (2, 1) and a pair whose last frame has no depth equals ygz_hip_stereo_odometry_slots on the same slots bit for bit
(T_rel, status, matches, inliers, retried, the match list per last feature); _TCW is written for the pairs that pass _min_tracked, as T_rel o
last's pose and carried along the chain, and for no other; with _min_tracked out of reach nothing is written; Track of one pair equals its
entry in the batch; no _mappoint, no map point and no keyframe appears."""
import os
import subprocess

import numpy as np
import pytest

import stereo_ref as sr
import svo_ref as sv

pytestmark = pytest.mark.gpu
W, H, SHIFT, Z = 320, 240, 3, 4.0
POSE0 = np.array([0.01, -0.02, 0.005, 0.0, 0.3, -0.2, 1.0])
POSE0[3] = np.sqrt(1.0 - np.sum(POSE0[:3] ** 2))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_svo_surface_build import build_program
    d = str(tmp_path_factory.mktemp("svo_gpu"))
    exe = build_program(d)
    rng = np.random.default_rng(31)
    src = sr.texture(W + 2 * SHIFT, H, 6)
    px0, level = sr.lattice(W + 2 * SHIFT, H, 12)
    angle = rng.uniform(0, 360, len(level))
    n = []
    for k in range(3):
        x = px0[:, 0] - k * SHIFT
        keep = np.flatnonzero((x >= 12) & (x <= W - 12))
        np.ascontiguousarray(src[:, k * SHIFT:k * SHIFT + W]).tofile(os.path.join(d, "img%d.bin" % k))
        np.stack([x[keep], px0[keep, 1]], 1).astype(np.float64).tofile(os.path.join(d, "k%d_px.bin" % k))
        level[keep].astype(np.int32).tofile(os.path.join(d, "k%d_level.bin" % k))
        angle[keep].astype(np.float64).tofile(os.path.join(d, "k%d_angle.bin" % k))
        np.where(rng.uniform(size=len(keep)) < 0.7, Z, -1.0).tofile(os.path.join(d, "k%d_depth.bin" % k))
        n.append(len(keep))
    POSE0.tofile(os.path.join(d, "pose0.bin"))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return (lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)), n


def test_batch_equals_the_c_call(out):
    read, n = out
    res = read("batch_res", np.int32).reshape(3, 5)
    counts, cells = read("abi_counts", np.int32).reshape(3, 8), len(read("abi_match", np.int32)) // 3
    assert read("batch_trel", np.float64).tobytes() == read("abi_trel", np.float64).tobytes()
    assert np.array_equal(res[:, 0], read("abi_status", np.int32)) and np.array_equal(res[:, 1], counts[:, 3])
    assert np.array_equal(res[:, 2], read("abi_inliers", np.int32)) and np.array_equal(res[:, 3], counts[:, 7])
    match = read("abi_match", np.int32).reshape(3, cells)
    for p, m in enumerate((n[0], n[1], n[0])):
        got = read("batch_match%d" % p, np.int32)
        assert len(got) == m == counts[p, 0] and np.array_equal(got, match[p, :m]) and (match[p, m:] == -1).all()
    # the case is about something: two pairs tracked with many inliers, the blind one failed after its retry
    assert res[:2, 0].tolist() == [0, 0] and (res[:2, 1] > 50).all() and (res[:2, 2] > 30).all()
    assert res[2].tolist() == [1, 0, 0, 1, 0] and counts[2, 1] == 0
    assert np.abs(read("batch_trel", np.float64).reshape(3, 7)[:2, 4] + SHIFT * Z / 520.9).max() < 2e-3


def test_poses_written_only_for_tracked_pairs(out):
    read, _ = out
    res = read("batch_res", np.int32).reshape(3, 5)
    trel, poses = read("batch_trel", np.float64).reshape(3, 7), read("batch_poses", np.float64).reshape(5, 7)
    assert read("batch_ret", np.int32)[0] == 2 and res[:, 4].tolist() == [1, 1, 0]
    assert np.array_equal(res[:, 4] == 1, (res[:, 0] == 0) & (res[:, 2] >= 10))
    same = lambda a, b: np.allclose(a, b, atol=1e-12) or np.allclose(a, np.concatenate([-b[:4], b[4:]]), atol=1e-12)
    assert poses[0].tobytes() == POSE0.tobytes() and poses[4].tobytes() == POSE0.tobytes()
    assert same(poses[1], sv.se3_mul(trel[0], POSE0)) and same(poses[2], sv.se3_mul(trel[1], sv.se3_mul(trel[0], POSE0)))
    assert poses[3].tobytes() == sv.IDENTITY.tobytes()                    # the pair that failed left its current frame alone
    # _min_tracked out of reach: the same results, nothing written
    strict, sposes = read("strict_res", np.int32).reshape(2, 5), read("strict_poses", np.float64).reshape(5, 7)
    assert read("strict_ret", np.int32)[0] == 0 and np.array_equal(strict[:, :4], res[:2, :4]) and strict[:, 4].tolist() == [0, 0]
    assert read("strict_trel", np.float64).tobytes() == trel[:2].tobytes()
    assert sposes[1].tobytes() == sv.IDENTITY.tobytes() and sposes[2].tobytes() == sv.IDENTITY.tobytes() and sposes[0].tobytes() == POSE0.tobytes()


def test_single_pair_equals_its_batch_entry(out):
    read, _ = out
    res, one = read("batch_res", np.int32).reshape(3, 5), read("single_res", np.int32).reshape(1, 5)
    assert np.array_equal(one[0], res[0]) and read("single_ret", np.int32)[0] == 1
    assert read("single_trel", np.float64).tobytes() == read("batch_trel", np.float64)[:7].tobytes()
    assert np.array_equal(read("single_match0", np.int32), read("batch_match0", np.int32))
    assert read("single_poses", np.float64).reshape(5, 7)[1].tobytes() == read("batch_poses", np.float64).reshape(5, 7)[1].tobytes()


def test_no_map_is_touched(out):
    read, _ = out
    assert read("untouched", np.int32).tolist() == [1]
