"""More distinct frames in one call than the runtime keeps resident, on the MI355X: tests/cpp/svo_resident.cpp in a subprocess under a time
limit with YGZ_HIP_MAX_FRAMES=2, on three QVGA frames whose pictures move by 3 pixels per frame (tests/stereo_ref.py's texture) with a dozen
lattice keypoints each, all on level 0 and all with the scene's depth.

StereoOdometry::TrackPairs over (1, 0), (2, 1) needs three slots: the slot loader the three slot trackers share (host/surface_share.cpp) sees
the third frame take the first one's slot and refuses; the call returns 0 with its results cleared and every _TCW is bitwise what it was.
The single pair (1, 0) afterwards fits and comes back through the device: a Result with a match entry per feature of frame 0.  Its twelve
keypoints are the same scene points a whole number of level-0 pixels apart, inside the 7 pixel window, so at least the 6 matches the program
asks for are found and the status is 0."""
import os
import subprocess

import numpy as np
import pytest

import stereo_ref as sr
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "ygz_slam_amd")
W, H, SHIFT, Z, STEP = 320, 240, 3, 4.0, 64
POSE0 = np.array([0.01, -0.02, 0.005, 0.0, 0.3, -0.2, 1.0])
POSE0[3] = np.sqrt(1.0 - np.sum(POSE0[:3] ** 2))
IDENTITY = np.array([0, 0, 0, 1.0, 0, 0, 0])


def test_three_frames_on_two_slots_are_refused_and_two_still_track(tmp_path):
    d = str(tmp_path)
    exe = os.path.join(d, "svo_resident")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "svo_resident.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    rng = np.random.default_rng(37)
    src = sr.texture(W + 2 * SHIFT, H, 6)
    px0, _ = sr.lattice(W + 2 * SHIFT, H, STEP)
    angle = rng.uniform(0, 360, len(px0))
    for k in range(3):
        x = px0[:, 0] - k * SHIFT
        keep = np.flatnonzero((x >= 12) & (x <= W - 12))
        assert len(keep) == 12
        np.ascontiguousarray(src[:, k * SHIFT:k * SHIFT + W]).tofile(os.path.join(d, "img%d.bin" % k))
        np.stack([x[keep], px0[keep, 1]], 1).astype(np.float64).tofile(os.path.join(d, "k%d_px.bin" % k))
        np.zeros(len(keep), np.int32).tofile(os.path.join(d, "k%d_level.bin" % k))
        angle[keep].astype(np.float64).tofile(os.path.join(d, "k%d_angle.bin" % k))
        np.full(len(keep), Z).tofile(os.path.join(d, "k%d_depth.bin" % k))
    POSE0.tofile(os.path.join(d, "pose0.bin"))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120, env=dict(os.environ, YGZ_HIP_MAX_FRAMES="2"))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    read = lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)
    # the refusal: 0, no result, no pose touched
    before = read("before_poses", np.float64)
    assert before.tobytes() == np.concatenate([POSE0, IDENTITY, IDENTITY]).tobytes()
    assert read("refused", np.int32).tolist() == [0, 0] and read("refused_poses", np.float64).tobytes() == before.tobytes()
    assert "more distinct frames than the runtime keeps resident" in r.stderr + r.stdout
    # two frames afterwards: through the device
    ret, status, matches, inliers, retried, written = read("single_res", np.int32).tolist()
    match, poses = read("single_match", np.int32), read("single_poses", np.float64).reshape(3, 7)
    assert status == 0 and 6 <= matches <= 12 and len(match) == 12 and ((match >= -1) & (match < 12)).all() and (match >= 0).sum() >= 6
    assert ret == written == int(inliers >= 3) and retried in (0, 1)
    assert poses[0].tobytes() == POSE0.tobytes() and poses[2].tobytes() == IDENTITY.tobytes()
    assert (poses[1].tobytes() != IDENTITY.tobytes()) == bool(written)
