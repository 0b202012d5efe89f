"""Frame::InitFrame through the lens undistortion on the MI355X (ygz::hip::Runtime::UploadColor): with camera.k1, k2, p1, p2 set, level 0 of a
BGR frame and of a gray frame equals the restatement's image (tests/undist_ref.c) and level 1 the oracle's pyrDown of it; a frame evicted and
brought back from _color, and one brought back from the _pyramid[0] mirror (already undistorted: uploaded as it is), have the levels they had
before; PinholeCamera::DistortPoint is steps 2-3 of the spec; with the default configuration _pyramid[0] is the plain gray.  The program
tests/cpp/undist_surface.cpp runs in a subprocess under a time limit, with two frame slots so that frames are evicted."""
import os
import subprocess

import numpy as np
import pytest

import undist_ref as ur

pytestmark = pytest.mark.gpu

W, H = 160, 120


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_undistort_surface_build import build_program
    d = str(tmp_path_factory.mktemp("undist_gpu"))
    exe = build_program(d)
    env = dict(os.environ, YGZ_HIP_MAX_FRAMES="2")
    for mode in ("distorted", "default"):
        r = subprocess.run([exe, d, mode], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return lambda name, dtype=np.uint8: np.fromfile(os.path.join(d, name + ".bin"), dtype)


@pytest.fixture(scope="module")
def camera(out):
    c = out("camera", np.float32).astype(np.float64)
    cam = tuple(float(v) for v in c[4:])
    return cam, ur.params(cam, k1=c[0], k2=c[1], p1=c[2], p2=c[3])


def test_init_frame_undistorts(out, camera, oracle):
    cam, p = camera
    assert (p.k1, p.k2, p.p1, p.p2) == tuple(float(np.float32(v)) for v in (0.2624, -0.9531, -0.0054, 0.0026))
    a, b = out("a_color").reshape(H, W, 3), out("b_color").reshape(H, W)
    want_a, want_b = ur.undistort(a, p, cam), ur.undistort(b, p, cam)
    assert not np.array_equal(want_a, ur.gray_of(a))                               # the case is about something
    assert np.array_equal(out("a_before_l0").reshape(H, W), want_a) and np.array_equal(out("a_mirror_l0").reshape(H, W), want_a)
    assert np.array_equal(out("b_before_l0").reshape(H, W), want_b)
    assert np.array_equal(out("a_before_l1").reshape(H // 2, W // 2), oracle.pyr_down(want_a))
    assert np.array_equal(out("b_before_l1").reshape(H // 2, W // 2), oracle.pyr_down(want_b))


@pytest.mark.parametrize("frame", ["a", "b"])
def test_an_evicted_frame_comes_back_as_it_was(out, frame):
    """a: from _color, undistorted again; b: from the _pyramid[0] mirror, never remapped twice"""
    for level in ("l0", "l1"):
        assert np.array_equal(out("%s_after_%s" % (frame, level)), out("%s_before_%s" % (frame, level))), level


def test_distort_point(out, camera):
    _, p = camera
    assert tuple(out("distort_point", np.float64)) == ur.distort_point(p, 0.31, -0.22)


def test_default_configuration_is_the_plain_gray(out):
    color = out("default_color").reshape(480, 640, 3)
    assert np.array_equal(out("default_l0").reshape(480, 640), ur.gray_of(color))
