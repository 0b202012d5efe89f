"""ygz::StereoLocalMap on the MI355X, through tests/cpp/slm_surface.cpp in a subprocess under a time limit.  The same small map is built
twice: three keyframes and four QVGA frames of a sequence whose pictures move by 3 pixels per frame (tests/stereo_ref.py's texture), lattice
keypoints that move with them, 70 % with the scene's constant depth, a third of every frame's features already holding the map point a
motion-model stage would have left; the fourth frame has 12 features only.  On one copy StereoTracker::TrackLocalMap runs frame by frame with
the right columns PoseOptimizer::URightFromDepth gives for the same depths; on the other ONE StereoLocalMap::TrackLocalMap call runs.  _TCW
(bitwise), the map point behind every feature, Feature::_bad, Feature::_depth, and _cnt_visible, _cnt_found and _track_in_view of every map point
must be equal; the short frame is reported as not tracked; no map point or keyframe appears; a single-frame call equals its batch entry."""
import os
import subprocess

import numpy as np
import pytest

import popt_ref
import stereo_ref as sr
from conftest import make_ctx

pytestmark = pytest.mark.gpu
W, H, SHIFT, Z, NF = 320, 240, 3, 4.0, 4
K = popt_ref.DEFAULT_K
KF_AT = (0, 1, 3)                                                      # the keyframes stand where frames 0, 1 and 3 do


def pose(k, off=0.0):
    return np.array([0, 0, 0, 1.0, (-k * SHIFT + off) * Z / K[0], 0, 0])


@pytest.fixture(scope="module")
def out(tmp_path_factory, hip_lib):
    from test_slm_surface_build import build_program
    d = str(tmp_path_factory.mktemp("slm_gpu"))
    exe = build_program(d)
    rng = np.random.default_rng(41)
    src = sr.texture(W + 3 * SHIFT, H, 6)
    px0, level = sr.lattice(W + 3 * SHIFT, H, 12)
    angle = rng.uniform(0, 360, len(level))
    P = len(level)
    # the map points: the lattice at the scene's depth, in the first camera's frame
    mp_pos = np.stack([(px0[:, 0] - K[2]) / K[0] * Z, (px0[:, 1] - K[3]) / K[1] * Z, np.full(P, Z)], 1)
    inside = lambda k: np.flatnonzero((px0[:, 0] - k * SHIFT >= 12) & (px0[:, 0] - k * SHIFT <= W - 12))
    # the keyframes' features with the descriptors the device computes for them
    ctx = make_ctx(hip_lib, width=W, height=H, levels=3, max_frames=2)
    kft = dict(kf=[], level=[], mp=[], px=[], desc=[])
    seen_by_kf1 = None
    for j, k in enumerate(KF_AT):
        keep = inside(k)
        keep = keep[rng.uniform(size=len(keep)) < 0.7]
        if j == 1:
            seen_by_kf1 = set(keep.tolist())
        ctx.upload_gray(0, np.ascontiguousarray(src[:, k * SHIFT:k * SHIFT + W]))
        ctx.build_pyramid(0, 1)
        p = np.stack([px0[keep, 0] - k * SHIFT, px0[keep, 1]], 1)
        ctx.describe_given_angle(0, p, level[keep].astype(np.int32), angle[keep].astype(np.float32))
        kp = ctx.get_keypoints_batch(0, 1)
        assert int(kp["count"][0]) == len(keep)
        kft["kf"].append(np.full(len(keep), j)); kft["level"].append(level[keep]); kft["mp"].append(keep); kft["px"].append(p)
        kft["desc"].append(kp["desc"][0, :len(keep)])
    ctx.close()
    np.stack([pose(k) for k in KF_AT]).tofile(os.path.join(d, "kf_poses.bin"))
    for name, t in (("kf", np.int32), ("level", np.int32), ("mp", np.int32), ("px", np.float64), ("desc", np.uint8)):
        np.ascontiguousarray(np.concatenate(kft[name]), t).tofile(os.path.join(d, "kft_%s.bin" % name))
    mp_pos.tofile(os.path.join(d, "mp_pos.bin"))
    n, held = [], []
    for k in range(NF):
        keep = inside(k)
        if k == 3:
            keep = keep[:12]
        np.ascontiguousarray(src[:, k * SHIFT:k * SHIFT + W]).tofile(os.path.join(d, "img%d.bin" % k))
        np.stack([px0[keep, 0] - k * SHIFT, px0[keep, 1]], 1).astype(np.float64).tofile(os.path.join(d, "f%d_px.bin" % k))
        level[keep].astype(np.int32).tofile(os.path.join(d, "f%d_level.bin" % k))
        angle[keep].astype(np.float64).tofile(os.path.join(d, "f%d_angle.bin" % k))
        np.where(rng.uniform(size=len(keep)) < 0.7, Z, -1.0).tofile(os.path.join(d, "f%d_depth.bin" % k))
        # what a motion-model stage left: a third of the features hold their point, if keyframe 1 (which is in both lists) observes it
        mp = np.where((rng.uniform(size=len(keep)) < 1 / 3) & np.array([i in seen_by_kf1 for i in keep.tolist()]), keep, -1).astype(np.int32)
        mp.tofile(os.path.join(d, "f%d_mp.bin" % k))
        pose(k, 0.4).tofile(os.path.join(d, "f%d_pose.bin" % k))
        n.append(len(keep)); held.append(int((mp >= 0).sum()))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return (lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)), n, held, P


def test_one_call_equals_the_tracker_frame_by_frame(out):
    read, n, held, P = out
    assert read("batch_pose", np.float64).tobytes() == read("old_pose", np.float64).tobytes()
    for k in range(NF):
        for name, t in (("feat", np.int32), ("bad", np.uint8), ("depth", np.uint64)):
            a, b = read("old_%s%d" % (name, k), t), read("batch_%s%d" % (name, k), t)
            assert len(a) == n[k] and np.array_equal(a, b), (name, k)
    a, b = read("old_mp", np.int32).reshape(P, 3), read("batch_mp", np.int32).reshape(P, 3)
    assert np.array_equal(a, b)
    # the case is about something: many new associations on the three full frames, poses that moved, points seen, found and not in view
    res = read("batch_ret", np.int32)[1:].reshape(NF, 5)
    assert held[0] > 30 and (res[:3, 1] > 50).all() and (res[:3, 2] == res[:3, 1] + np.array(held[:3])).all() and (res[:3, 3] > 60).all()
    entry = np.stack([pose(k, 0.4) for k in range(NF)])
    got = read("batch_pose", np.float64).reshape(NF, 7)
    assert (np.abs(got[:3] - entry[:3]).max(1) > 1e-5).all() and np.abs(got[:3, 4] - np.stack([pose(k) for k in range(3)])[:, 4]).max() < 2e-3
    assert (a[:, 0] > 1).sum() > 100 and (a[:, 1] > 1).sum() > 100 and 0 < a[:, 2].sum() < P
    old_ret = read("old_ret", np.int32)
    for k in range(NF):                                                  # the tracker's return value: features with a point that are not outliers
        feat, bad = read("batch_feat%d" % k, np.int32), read("batch_bad%d" % k, np.uint8)
        assert old_ret[k] == ((feat >= 0) & (bad == 0)).sum()


def test_a_frame_below_min_tracked_is_reported(out):
    read, n, held, _ = out
    ret = read("batch_ret", np.int32)
    res = ret[1:].reshape(NF, 5)
    assert n[3] == 12 and res[3, 3] < 30 and res[3, 4] == 0 and res[:3, 4].tolist() == [1, 1, 1] and ret[0] == 3
    assert np.array_equal(res[:, 4] == 1, (res[:, 0] == 0) & (res[:, 3] >= 30))


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
