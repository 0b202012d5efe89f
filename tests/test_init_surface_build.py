"""ygz::Initializer (include/ygz/Algorithm/Initializer.h, libygz_host.so) without a device: a program written against include/ygz only, calling
TryInitialize, GetT21, GetTriangluatedPoints and ba::TwoViewBACeres in the order of src/Module/VisualOdometry.cpp:133-151, compiles and links
with -Wl,--no-undefined against both libraries; the public surface matches the reference's; the new C ABI symbols are bound by the loader."""
import os
import re
import subprocess

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/init_surface.cpp into out_dir (also used by tests/test_gpu_initializer.py to run it on the device)"""
    exe = os.path.join(out_dir, "init_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "init_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_initializer_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    assert os.path.exists(exe)


def test_public_surface_as_the_reference_declares_it():
    h = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "Initializer.h")).read()
    for decl in [r"bool\s+TryInitialize\s*\(\s*vector<Vector2d>\s*&\s*px1\s*,\s*vector<Vector2d>\s*&\s*px2\s*,\s*Frame\s*\*\s*ref\s*,\s*Frame\s*\*\s*curr\s*\)",
                 r"SE3\s+GetT21\s*\(\s*\)\s*const", r"void\s+GetTriangluatedPoints\s*\(\s*vector<Vector3d>\s*&\s*pts_3d\s*,\s*vector<bool>\s*&\s*inliers\s*\)",
                 r"float\s+_sigma\s*=\s*2\.0;", r"float\s+_sigma2\s*=\s*4\.0;", r"int\s+_max_iter\s*=\s*200;", r"double\s+_min_parallex\s*=\s*1\.0;",
                 r"int\s+_min_triangulated_pts\s*=\s*8;", r"double\s+good_point_ratio_H\s*=\s*0\.9;", r"\}\s*_options;"]:
        assert re.search(decl, h), decl
    assert '#include "ygz/Algorithm/Initializer.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()


def test_init_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    for s in hip_lib.INIT_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    p = hip_lib.default_init_params()
    assert (p.sigma, p.sigma2, p.max_iter, p.min_parallax, p.min_triangulated) == (2.0, 4.0, 200, 1.0, 8) and abs(p.good_point_ratio_h - 0.9) < 1e-15


def test_init_entry_points_refuse_bad_arguments_without_device(hip_lib):
    """n < 8 and a null context are refused before any device is touched; the sample sets are a host function"""
    import ctypes
    import numpy as np
    lib = hip_lib.load()
    px = np.zeros((4, 2))
    res = hip_lib.InitResult()
    K = (ctypes.c_double * 4)(500, 500, 320, 240)
    lib.ygz_hip_initialize.argtypes = None
    assert lib.ygz_hip_initialize(None, px.ctypes.data_as(ctypes.c_void_p), px.ctypes.data_as(ctypes.c_void_p), 4, K, None,
                                  ctypes.byref(res), None, None) == hip_lib.E_INVALID
    with __import__("pytest").raises(hip_lib.YgzHipError):
        hip_lib.init_sample_sets(7, 200)
    s = hip_lib.init_sample_sets(8, 3)
    assert s.shape == (3, 8) and all(sorted(r) == list(range(8)) for r in s.tolist())
