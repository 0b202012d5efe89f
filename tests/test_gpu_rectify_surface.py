"""ygz::StereoRig on the MI355X (include/ygz/Basic/StereoRig.h, ygz_slam_amd/host/ygz_rectify.cpp): after InitPair level 0 of both frames is the
restatement's rectified picture (tests/rect_ref.c + undist_ref's remap) for BGR and gray pictures, and level 1 the oracle's pyrDown of it; a
frame evicted and brought back from _color (rectified again), and one brought back from the _pyramid[0] mirror (already rectified: uploaded as
it is), have the levels they had; frames made with plain InitFrame are untouched by the rig; R1, R2 and the baseline are the restatement's;
ComputeStereoMatches after InitPair equals the stereo restatement on the rectified levels and sets the depths of the raw textured pair.  The
program tests/cpp/rect_surface.cpp runs in subprocesses under a time limit, with two frame slots so that frames are evicted."""
import os
import subprocess

import numpy as np
import pytest

import rect_ref as rr
import stereo_ref as sr
import undist_ref as ur

pytestmark = pytest.mark.gpu

W, H = 160, 120
SMALL = tuple(float(np.float32(v)) for v in (130.2, 130.3, 81.3, 62.4))
BORDER = 9


def calib(w, h, cam, border):
    l0, l1 = rr.rig_lenses(cam, border)
    lens = [[l.fx, l.fy, l.cx, l.cy, l.k1, l.k2, l.p1, l.p2, l.k3] for l in (l0, l1)]
    return np.array([w, h, *cam, *lens[0], *lens[1], *rr.RIG_R.reshape(9), *rr.RIG_T, border], np.float64)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from test_rectify_surface_build import build_program
    return build_program(str(tmp_path_factory.mktemp("rect_exe")))


def run(exe, d, mode):
    env = dict(os.environ, YGZ_HIP_MAX_FRAMES="2")
    r = subprocess.run([exe, d, mode], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return lambda name, dtype=np.uint8: np.fromfile(os.path.join(d, name + ".bin"), dtype)


@pytest.fixture(scope="module", params=["bgr", "gray"])
def pair(request, exe, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rect_" + request.param))
    ch = 3 if request.param == "bgr" else 1
    pics = {n: ur.picture(W, H, 90 + i, channels=ch) for i, n in enumerate(("left", "right", "c", "e"))}
    for n, p in pics.items():
        p.tofile(os.path.join(d, n + ".bin"))
    calib(W, H, SMALL, BORDER).tofile(os.path.join(d, "calib.bin"))
    return run(exe, d, request.param), pics


def rig_params(out, cam, border):
    rig = out("rig", np.float64)
    R1, R2, b = rr.stereo_rectify(rr.RIG_R, rr.RIG_T)
    assert np.array_equal(rig[:9].reshape(3, 3), R1) and np.array_equal(rig[9:18].reshape(3, 3), R2) and rig[18] == b and rig[19] == cam[0] * b
    l0, l1 = rr.rig_lenses(cam, border)
    return rr.params(l0, R1), rr.params(l1, R2), b


def test_init_pair_rectifies(pair, oracle):
    out, pics = pair
    p0, p1, _ = rig_params(out, SMALL, BORDER)
    want = {"l": rr.rectify(pics["left"], p0, SMALL), "r": rr.rectify(pics["right"], p1, SMALL)}
    gray = ur.gray_of(pics["left"]) if pics["left"].ndim == 3 else pics["left"]
    assert not np.array_equal(want["l"], gray)                                       # the case is about something
    for k in ("l", "r"):
        assert np.array_equal(out(k + "_before_l0").reshape(H, W), want[k]), k
        assert np.array_equal(out(k + "_before_l1").reshape(H // 2, W // 2), oracle.pyr_down(want[k])), k
    assert np.array_equal(out("l_mirror_l0").reshape(H, W), want["l"])


@pytest.mark.parametrize("frame", ["l", "r"])
def test_an_evicted_frame_comes_back_as_it_was(pair, frame):
    """l: from _color, rectified again; r: from the _pyramid[0] mirror, never remapped twice"""
    out, _ = pair
    for level in ("l0", "l1"):
        assert np.array_equal(out("%s_after_%s" % (frame, level)), out("%s_before_%s" % (frame, level))), level


def test_plain_frames_are_untouched_by_the_rig(pair):
    out, pics = pair
    plain = (lambda p: ur.gray_of(p) if p.ndim == 3 else p)
    assert np.array_equal(out("c_l0").reshape(H, W), plain(pics["c"])) and np.array_equal(out("e_l0").reshape(H, W), plain(pics["e"]))
    assert np.array_equal(out("l_plain_l0").reshape(H, W), plain(pics["left"]))      # a plain InitFrame ends the membership


def test_stereo_matches_after_init_pair(exe, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("rect_stereo"))
    left, right, _, _ = rr.textured_raw_pair()
    left.tofile(os.path.join(d, "raw_left.bin"))
    right.tofile(os.path.join(d, "raw_right.bin"))
    calib(rr.RIG_W, rr.RIG_H, ur.DEFAULT_CAMERA, 0).tofile(os.path.join(d, "calib.bin"))
    out = run(exe, d, "stereo")
    p0, p1, b = rig_params(out, ur.DEFAULT_CAMERA, 0)
    shapes = [(480, 640), (240, 320), (120, 160)]
    levels = {k: [out("%s_l%d" % (k, L)).reshape(shapes[L]) for L in range(3)] for k in ("sl", "sr")}
    assert np.array_equal(levels["sl"][0], rr.rectify(left, p0)) and np.array_equal(levels["sr"][0], rr.rectify(right, p1))
    kl, kr = [sr.keypoints(out(s + "_px", np.float64), out(s + "_level", np.int32), out(s + "_desc")) for s in ("l", "r")]
    ref = sr.match(levels["sl"], levels["sr"], kl, kr, sr.params(baseline=b))
    status, depth, u_right = out("status", np.int32), out("depth", np.float64), out("u_right", np.float64)
    ok = ref["status"] == sr.OK
    assert np.array_equal(status, ref["status"]) and out("count", np.int32)[0] == ok.sum()
    assert np.array_equal(depth[ok], ref["depth"][ok]) and (depth[~ok] == -1).all()
    assert np.array_equal(u_right[ok], ref["u_right"][ok]) and (u_right[~ok] == -1).all()
    share = ok.mean()
    good = (np.abs(kl["px"][ok, 0] - u_right[ok] - rr.RIG_D) < 1.0).mean()
    print("InitPair + ComputeStereoMatches: %d of %d features get a depth (%.3f), %.3f of them within 1 px of 20" % (ok.sum(), len(ok), share, good))
    assert share >= 0.45 and good >= 0.99
    assert abs(np.median(depth[ok]) / (sr.DEFAULT_FX * b / rr.RIG_D) - 1.0) < 0.01
