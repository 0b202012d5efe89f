"""ygz::StereoRefTracker on the MI355X, through tests/cpp/srk_surface.cpp in a subprocess under a time limit.  The same small map is built
twice: two keyframes and four QVGA frames of a sequence whose pictures move by 3 pixels per frame (tests/stereo_ref.py's texture), lattice
keypoints that move with them, 70 % with the scene's constant depth, 70 % of a keyframe's features carrying the scene's point under them; the
fourth frame has 12 features only.  On one copy the host route runs frame by frame: Matcher::SearchByBoW with checkOrientation off, the claim
of ygz_reloc.cpp, _mappoint, PoseOptimizer::Optimize with PoseOptimizer::URightFromDepth, bad features dropped; on the other ONE
StereoRefTracker::TrackReferenceKeyFrame call runs with _check_orientation off.  _TCW (bitwise), the map point behind every feature,
Feature::_bad and Feature::_depth (bitwise) must be equal, and no _cnt_found moves; the short frame is reported as not tracked; no map point
or keyframe appears; a single-frame call equals its batch entry.  The vocabulary (k = 4, L = 6) leaves at least 8 distinct nodes at levelsup
4."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import popt_ref
import stereo_ref as sr

pytestmark = pytest.mark.gpu
W, H, SHIFT, Z, NF = 320, 240, 3, 4.0, 4
K = popt_ref.DEFAULT_K
KF_AT = (0, 2)                                                         # the keyframes stand where frames 0 and 2 do
KF_OF = (0, 0, 1, 1)


def pose(k, off=0.0):
    return np.array([0, 0, 0, 1.0, (-k * SHIFT + off) * Z / K[0], 0, 0])


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_srk_surface_build import build_program
    d = str(tmp_path_factory.mktemp("srk_gpu"))
    exe = build_program(d)
    rng = np.random.default_rng(43)
    src = sr.texture(W + 3 * SHIFT, H, 6)
    px0, level = sr.lattice(W + 3 * SHIFT, H, 12)
    angle = rng.integers(0, 1440, len(level)) / 4.0
    P = len(level)
    # the map points: the lattice at the scene's depth, in the first camera's frame
    mp_pos = np.stack([(px0[:, 0] - K[2]) / K[0] * Z, (px0[:, 1] - K[3]) / K[1] * Z, np.full(P, Z)], 1)
    inside = lambda k: np.flatnonzero((px0[:, 0] - k * SHIFT >= 12) & (px0[:, 0] - k * SHIFT <= W - 12))
    with open(os.path.join(d, "vocab.bin"), "wb") as f:
        f.write(fixtures.synthetic_vocabulary(k=4, L=6, seed=11))
    mp_pos.tofile(os.path.join(d, "mp_pos.bin"))

    def write(tag, k, keep, entry):
        np.ascontiguousarray(src[:, k * SHIFT:k * SHIFT + W]).tofile(os.path.join(d, tag + "_img.bin"))
        np.stack([px0[keep, 0] - k * SHIFT, px0[keep, 1]], 1).astype(np.float64).tofile(os.path.join(d, tag + "_px.bin"))
        level[keep].astype(np.int32).tofile(os.path.join(d, tag + "_level.bin"))
        angle[keep].astype(np.float64).tofile(os.path.join(d, tag + "_angle.bin"))
        np.where(rng.uniform(size=len(keep)) < 0.7, Z, -1.0).tofile(os.path.join(d, tag + "_depth.bin"))
        entry.tofile(os.path.join(d, tag + "_pose.bin"))
    carried = []
    for j, k in enumerate(KF_AT):
        keep = inside(k)
        write("k%d" % j, k, keep, pose(k))
        mp = np.where(rng.uniform(size=len(keep)) < 0.7, keep, -1).astype(np.int32)
        mp.tofile(os.path.join(d, "k%d_mp.bin" % j))
        carried.append(int((mp >= 0).sum()))
    n = []
    for k in range(NF):
        keep = inside(k)
        if k == 3:
            keep = keep[:12]
        write("f%d" % k, k, keep, pose(k, 0.4))
        n.append(len(keep))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return (lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)), n, carried, P


def test_one_call_equals_the_host_route_frame_by_frame(out):
    read, n, carried, P = out
    assert read("batch_pose", np.float64).tobytes() == read("old_pose", np.float64).tobytes()
    for k in range(NF):
        for name, t in (("feat", np.int32), ("bad", np.uint8), ("depth", np.uint64)):
            a, b = read("old_%s%d" % (name, k), t), read("batch_%s%d" % (name, k), t)
            assert len(a) == n[k] and np.array_equal(a, b), (name, k)
    assert np.array_equal(read("old_found", np.int32), read("batch_found", np.int32)) and (read("batch_found", np.int32) == 1).all()
    # the case is about something: many associations on the three full frames, poses that moved towards the truth
    res = read("batch_ret", np.int32)[1:].reshape(NF, 5)
    old = read("old_ret", np.int32).reshape(NF, 2)
    assert min(carried) > 100 and (res[:3, 1] > 60).all() and (res[:3, 2] > 50).all() and (res[:3, 0] == 0).all()
    assert np.array_equal(old[:3, 0], res[:3, 1]) and np.array_equal(old[:, 1], res[:, 3])
    entry = np.stack([pose(k, 0.4) for k in range(NF)])
    got = read("batch_pose", np.float64).reshape(NF, 7)
    assert (np.abs(got[:3] - entry[:3]).max(1) > 1e-5).all() and np.abs(got[:3, 4] - np.stack([pose(k) for k in range(3)])[:, 4]).max() < 2e-3
    for k in range(3):
        feat = read("batch_feat%d" % k, np.int32)
        assert (feat >= 0).sum() == res[k, 3] > 50 and (feat >= -1).all()


def test_the_vocabulary_is_deep_enough(out):
    read = out[0]
    assert read("nodes", np.int32)[0] >= 8


def test_the_short_frame_is_reported_as_not_tracked(out):
    read, n, _, _ = out
    ret = read("batch_ret", np.int32)
    res = ret[1:].reshape(NF, 5)
    assert n[3] == 12 and res[3].tolist() == [1, 0, 0, 0, 0] and res[:3, 4].tolist() == [1, 1, 1] and ret[0] == 3
    assert (read("batch_feat3", np.int32) == -1).all() and read("old_ret", np.int32).reshape(NF, 2)[3, 0] < 15
    assert read("batch_pose", np.float64).reshape(NF, 7)[3].tobytes() == pose(3, 0.4).tobytes()


def test_no_map_point_or_keyframe_appears(out):
    read = out[0]
    assert read("untouched", np.int32).tolist() == [1]


def test_single_frame_call_equals_its_batch_entry(out):
    read = out[0]
    one, res = read("single_ret", np.int32), read("batch_ret", np.int32)[1:].reshape(NF, 5)
    assert one[0] == 1 and np.array_equal(one[1:], res[1])
    assert read("single_pose", np.float64).reshape(NF, 7)[1].tobytes() == read("batch_pose", np.float64).reshape(NF, 7)[1].tobytes()
    for name, t in (("feat", np.int32), ("bad", np.uint8), ("depth", np.uint64)):
        assert np.array_equal(read("single_%s1" % name, t), read("batch_%s1" % name, t)), name
