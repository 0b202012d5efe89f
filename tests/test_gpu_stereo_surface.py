"""ygz::StereoMatcher on the MI355X: ComputeStereoMatches on scene a of tests/stereo_ref.py (320 x 240, three levels, shift 8, features on a
lattice) sets exactly the depths the array form ygz_hip_stereo_match returns for the same arrays -- which are the restatement's -- on the left
features with status OK, leaves every other Feature::_depth at -1, and returns their number.  The program tests/cpp/stereo_surface.cpp runs in a
subprocess under a time limit."""
import os
import subprocess

import numpy as np
import pytest

import stereo_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def out(tmp_path_factory, oracle):
    from test_stereo_surface_build import build_program
    d = str(tmp_path_factory.mktemp("stereo_gpu"))
    exe = build_program(d)
    s = sr.scene(oracle, "a")
    s.left[0].tofile(os.path.join(d, "left.bin"))
    s.right[0].tofile(os.path.join(d, "right.bin"))
    for side, k in (("l", s.kl), ("r", s.kr)):
        for name in ("px", "level", "desc"):
            k[name].tofile(os.path.join(d, "%s_%s.bin" % (side, name)))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return s, (lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype))


def test_compute_stereo_matches_sets_the_array_forms_depths(out):
    s, f = out
    n = len(s.kl["level"])
    depth, u_right, status = f("depth", np.float64), f("u_right", np.float64), f("status", np.int32)
    a_depth, a_ur, a_status = f("abi_depth", np.float64), f("abi_u_right", np.float64), f("abi_status", np.int32)
    assert len(depth) == len(a_depth) == n
    ok = a_status == sr.OK
    assert ok.sum() > 200 and (~ok).sum() > 50
    assert np.array_equal(status, a_status) and np.array_equal(depth[ok], a_depth[ok]) and (depth[~ok] == -1.0).all()
    assert np.array_equal(u_right, a_ur) and (u_right[~ok] == -1.0).all()
    assert list(f("count", np.int32)) == [int(ok.sum()), n]


def test_the_array_form_is_the_restatement(out):
    s, f = out
    fx = float(f("fx", np.float32)[0])
    want = sr.match(s.left, s.right, s.kl, s.kr, sr.params(baseline=0.25), fx=fx)
    assert np.array_equal(f("abi_depth", np.float64), want["depth"]) and np.array_equal(f("abi_u_right", np.float64), want["u_right"])
    assert np.array_equal(f("abi_status", np.int32), want["status"])
