"""The stereo-rectification surface without a device: tests/cpp/rect_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the C ABI symbols are bound by the loader and exported; ygz_rectify_params has the size and the fields of the
restatement's struct; every invalid call comes back YGZ_E_INVALID with a null context (the context is checked last, so a valid call with a
null context is refused too); ygz_hip_stereo_rectify, which is host code, equals the restatement bit for bit; the new sources read no
environment variable."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import rect_ref as rr
import undist_ref as ur
from test_rect_ref import random_rigs

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "rectify.hip"), os.path.join(PKG, "csrc", "remap_dev.h"), os.path.join(PKG, "host", "ygz_rectify.cpp"), os.path.join(ROOT, "tests", "cpp", "rect_surface.cpp"),
               os.path.join(ROOT, "include", "ygz", "Basic", "StereoRig.h")]


def build_program(out_dir):
    """compile tests/cpp/rect_surface.cpp into a program in out_dir (also used by tests/test_gpu_rectify_surface.py)"""
    exe = os.path.join(out_dir, "rect_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rect_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Basic", "StereoRig.h")).read()
    for decl in [r"bool\s+Rectify\s*\(\s*\)", r"const\s+double\s*\*\s*R1\s*\(\s*\)\s*const", r"const\s+double\s*\*\s*R2\s*\(\s*\)\s*const",
                 r"double\s+Baseline\s*\(\s*\)\s*const", r"double\s+bf\s*\(\s*\)\s*const", r"bool\s+InitPair\s*\(\s*Frame\s*\*\s*left\s*,\s*Frame\s*\*\s*right\s*\)"]:
        assert re.search(decl, hdr), decl
    assert '#include "ygz/Basic/StereoRig.h"' in open(os.path.join(ROOT, "include", "ygz", "Basic.h")).read()
    rt = open(os.path.join(ROOT, "include", "ygz", "hip", "Runtime.h")).read()
    assert re.search(r"void\s+SetRigCamera\s*\(\s*Frame\s*\*", rt) and re.search(r"int\s+RigCamera\s*\(\s*const\s+Frame\s*\*", rt)
    host = open(os.path.join(PKG, "host", "ygz_host.cpp")).read()
    # the re-upload of an evicted rig frame from _color is rectified in the one place every upload of _color goes through; the one from the
    # mirror stays a plain gray upload
    body = host[host.index("bool Runtime::UploadColor"):host.index("// HBM slot of a frame")]
    assert body.count("ygz_hip_build_pyramid_rectified(") == 1 and host.count("ygz_hip_build_pyramid_rectified(") == 1
    assert re.search(r"upload_gray\(c, slot, f->_pyramid\[0\]\.data[^\n]*ygz_hip_build_pyramid\(c, slot, 1, 0\)", host)
    assert "rig_camera.erase(f)" in host[host.index("void Runtime::Release"):host.index("void Runtime::RegisterLevels")]
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code, path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.RECTIFY_SYMBOLS == ["ygz_hip_stereo_rectify", "ygz_hip_default_rectify_params", "ygz_hip_set_rectification", "ygz_hip_rectify_map",
                                       "ygz_hip_build_pyramid_rectified"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: stereo rectification added", hdr) and hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for s in hip_lib.RECTIFY_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert re.search(r"#define\s+YGZ_RECT_CAMERAS\s+2\b", hdr) and hip_lib.RECT_CAMERAS == 2
    assert re.search(r"typedef struct \{\s*ygz_undistort_params\s+lens;[^}]*double\s+R\[9\];[^}]*\} ygz_rectify_params;", hdr)
    P = hip_lib.RectifyParams
    assert [n for n, _ in P._fields_] == [n for n, _ in rr.Params._fields_] == ["lens", "R"]
    assert ctypes.sizeof(P) == ctypes.sizeof(rr.Params) == rr.lib().rr_params_size() == 152
    assert P.lens.offset == rr.Params.lens.offset == 0 and P.R.offset == rr.Params.R.offset == rr.lib().rr_params_offset_R() == 80
    for (n, _), (rn, _) in zip(hip_lib.UndistortParams._fields_, ur.Params._fields_):
        assert getattr(hip_lib.UndistortParams, n).offset == getattr(ur.Params, rn).offset, n


def test_every_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.rectify_argtypes(lib)
    INV = hip_lib.E_INVALID
    good = dict(k1=0.1, k2=-0.2, p1=0.001, p2=-0.002, k3=0.3, fx=500.0, fy=501.0, cx=320.0, cy=240.0, border_value=0)

    def set_(camera=0, R=np.eye(3), **kw):
        v = dict(good, **kw)
        p = hip_lib.RectifyParams(hip_lib.UndistortParams(*[v[n] for n, _ in hip_lib.UndistortParams._fields_]),
                                  (ctypes.c_double * 9)(*[float(x) for x in np.asarray(R, np.float64).reshape(9)]))
        return lib.ygz_hip_set_rectification(None, camera, ctypes.byref(p))
    assert set_() == INV and set_(1, rr.RIG_R, border_value=255) == INV                # valid: only the context is missing
    for camera in (0, 1, -1, 2):
        assert lib.ygz_hip_set_rectification(None, camera, None) == INV               # dropping the map of no context
    assert set_(-1) == INV and set_(2) == INV
    for name in ("k1", "k2", "p1", "p2", "k3", "fx", "fy", "cx", "cy"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert set_(**{name: bad}) == INV, (name, bad)
    for bad in (dict(fx=0.0), dict(fy=0.0), dict(fx=-500.0), dict(fy=-1e-300), dict(border_value=-1), dict(border_value=256)):
        assert set_(**bad) == INV, bad
    for R in (np.eye(3) * 1.00001, np.diag([1.0, 1.0, -1.0]), np.zeros((3, 3)), np.full((3, 3), np.nan), np.diag([np.inf, 1.0, 1.0])):
        assert set_(R=R) == INV
    p = hip_lib.RectifyParams()
    p.lens.k1, p.lens.border_value, p.R[4] = 1.0, 77, 5.0
    assert lib.ygz_hip_default_rectify_params(None, ctypes.byref(p)) == INV
    assert (p.lens.k1, p.lens.fx, p.lens.border_value, p.R[4]) == (0.0, 0.0, 0, 0.0)   # zeroed all the same
    assert lib.ygz_hip_default_rectify_params(None, None) == INV
    q = np.zeros(4, np.int32)
    ip = q.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    for camera in (0, 1, -1, 2):
        assert lib.ygz_hip_rectify_map(None, camera, ip, ip) == INV and lib.ygz_hip_rectify_map(None, camera, None, None) == INV
    cams = (ctypes.c_uint8 * 2)(0, 1)
    bad_cams = (ctypes.c_uint8 * 2)(0, 2)
    for args in ((0, 1, 0, cams), (0, 2, 1, cams), (-1, 1, 0, cams), (0, 0, 0, cams), (0, 2, 0, bad_cams), (0, 2, 0, None)):
        assert lib.ygz_hip_build_pyramid_rectified(None, *args) == INV, args[:3]
    # ygz_hip_stereo_rectify: null arguments
    d = (ctypes.c_double * 9)(*np.eye(3).reshape(9))
    t = (ctypes.c_double * 3)(-0.1, 0.0, 0.0)
    o1, o2, b = (ctypes.c_double * 9)(), (ctypes.c_double * 9)(), ctypes.c_double(0)
    assert lib.ygz_hip_stereo_rectify(d, t, o1, o2, ctypes.byref(b)) == hip_lib.OK and b.value == 0.1
    for args in ((None, t, o1, o2, ctypes.byref(b)), (d, None, o1, o2, ctypes.byref(b)), (d, t, None, o2, ctypes.byref(b)),
                 (d, t, o1, None, ctypes.byref(b)), (d, t, o1, o2, None)):
        assert lib.ygz_hip_stereo_rectify(*args) == INV


def test_stereo_rectify_equals_the_restatement(hip_lib):
    """host code: no device, no context"""
    rigs = [(rr.RIG_R, rr.RIG_T)] + list(random_rigs(100, 11))
    for R, T in rigs:
        R1, R2, b = hip_lib.stereo_rectify(R, T)
        w1, w2, wb = rr.stereo_rectify(R, T)
        assert np.array_equal(R1, w1) and np.array_equal(R2, w2) and b == wb
    # the refusals agree too
    refused = [(rr.RIG_R, np.zeros(3)), (np.eye(3), [0.11, 0.0, 0.0]), (np.eye(3), [-0.01, 0.1, 0.0]), (rr.rodrigues((0.0, 2.2, 0.0)), rr.RIG_T),
               (rr.RIG_R * 1.00001, rr.RIG_T), (np.diag([1.0, 1.0, -1.0]), rr.RIG_T), (rr.RIG_R, [np.nan, 0.0, 0.0]), (np.full((3, 3), np.inf), rr.RIG_T)]
    lib = hip_lib.load()
    for R, T in refused:
        assert rr.stereo_rectify(R, T) is None
        a, t = np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(T, np.float64).reshape(3)
        o1, o2, b = np.zeros(9), np.zeros(9), ctypes.c_double(0)
        dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert lib.ygz_hip_stereo_rectify(dp(a), dp(t), dp(o1), dp(o2), ctypes.byref(b)) == hip_lib.E_INVALID
