"""ygz::LoopClosing (include/ygz/Algorithm/LoopClosing.h, libygz_host.so) and the Sim3 C ABI without a device: a program written against
include/ygz only (LoopClosing, Sim3) compiles and links with -Wl,--no-undefined; the public surface and its defaults are as declared; the new
C ABI symbols are bound by the loader; bad arguments are refused before a device is touched; the Sim3 algebra (compose, inverse, act) equals
numpy's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/loop_surface.cpp into a shared object in out_dir (also used by tests/test_gpu_loop_closing.py)"""
    so = os.path.join(out_dir, "libloop_surface.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "loop_surface.cpp"), "-o", so, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return so


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    return ctypes.CDLL(build_program(str(tmp_path_factory.mktemp("loop"))))


def test_loop_program_compiles_and_links(program):
    assert hasattr(program, "loop_run") and hasattr(program, "loop_sim3_algebra")


def test_public_surface():
    h = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "LoopClosing.h")).read()
    for decl in [r"class\s+LoopClosing\b", r"struct\s+Sim3\b",
                 r"bool\s+DetectLoop\s*\(\s*Frame\s*\*\s*kf\s*,\s*const\s+vector<Frame\s*\*>\s*&\s*keyframes\s*\)",
                 r"bool\s+DetectLoop\s*\(\s*Frame\s*\*\s*kf\s*\)", r"bool\s+ComputeSim3\s*\(\s*\)",
                 r"Frame\s*\*\s*GetMatchedKeyframe\s*\(\s*\)\s*const", r"const\s+Sim3\s*&\s*GetSim3\s*\(\s*\)\s*const",
                 r"const\s+Sim3\s*&\s*GetCorrectedPose\s*\(\s*\)\s*const",
                 r"const\s+vector<pair<MapPoint\s*\*\s*,\s*MapPoint\s*\*>>\s*&\s*GetMatches\s*\(\s*\)\s*const",
                 r"const\s+Stats\s*&\s*GetStats\s*\(\s*\)\s*const",
                 r"int\s+_min_kf_gap\s*=\s*10;", r"int\s+_consistency_th\s*=\s*3;", r"double\s+_min_common_words_ratio\s*=\s*0\.8;",
                 r"double\s+_acc_score_ratio\s*=\s*0\.75;", r"int\s+_acc_covisibles\s*=\s*10;", r"float\s+_knn_ratio\s*=\s*0\.75f;",
                 r"int\s+_min_bow_matches\s*=\s*20;", r"int\s+_ransac_iterations\s*=\s*300;", r"double\s+_ransac_chi2\s*=\s*9\.210;",
                 r"int\s+_min_inliers\s*=\s*20;", r"double\s+_refine_chi2\s*=\s*10;", r"bool\s+_fix_scale\s*=\s*false;", r"\}\s*_option;",
                 r"Sim3\s+inverse\s*\(\s*\)\s*const", r"void\s+to8\s*\(", r"static\s+Sim3\s+from8\s*\("]:
        assert re.search(decl, h), decl
    assert '#include "ygz/Algorithm/LoopClosing.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_loop.cpp") == 2


def test_sim3_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    for s in hip_lib.SIM3_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    p = hip_lib.default_sim3_params()
    assert (p.max_iter, p.chi2, p.min_inliers, p.chi2_refine, p.iters_first, p.iters_more, p.iters_again, p.fix_scale) == (300, 9.210, 20, 10.0, 5, 10, 5, 0)
    assert ctypes.sizeof(hip_lib.Sim3Result) == 168
    assert not hasattr(lib, "ygz_hip_sim3_sample_sets")          # the P3P RANSAC's sets serve both


def test_sim3_entry_points_refuse_bad_arguments_without_device(hip_lib):
    lib = hip_lib.load()
    X, u, lv = np.zeros((8, 3)), np.zeros((8, 2)), np.zeros((8, 2), np.int32)
    K = (ctypes.c_double * 4)(500, 500, 320, 240)
    res = (hip_lib.Sim3Result * 2)()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    off = np.array([0, 8], np.int32)
    lib.ygz_hip_sim3_ransac.argtypes = None
    assert lib.ygz_hip_sim3_ransac(None, 1, vp(off), vp(X), vp(X), vp(u), vp(u), vp(lv), K, None, res, None) == hip_lib.E_INVALID
    lib.ygz_hip_sim3_hypotheses.argtypes = None
    assert lib.ygz_hip_sim3_hypotheses(None, vp(X), vp(X), vp(u), vp(u), vp(lv), 8, K, None, None, None, None) == hip_lib.E_INVALID


def _q2R(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _M(S):
    M = np.eye(4)
    M[:3, :3] = S[7] * _q2R(S[:4])
    M[:3, 3] = S[4:7]
    return M


def test_sim3_algebra_against_numpy(program):
    rng = np.random.default_rng(8)
    program.loop_sim3_algebra.argtypes = [ctypes.c_void_p] * 4
    for _ in range(50):
        a = np.concatenate([rng.normal(size=4), rng.normal(size=3), [rng.uniform(0.3, 3)]])
        a[:4] /= np.linalg.norm(a[:4])
        b = np.concatenate([rng.normal(size=4), rng.normal(size=3), [rng.uniform(0.3, 3)]])
        b[:4] /= np.linalg.norm(b[:4])
        p = rng.normal(size=3)
        out = np.zeros(27)
        vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
        program.loop_sim3_algebra(vp(a), vp(b), vp(p), vp(out))
        assert np.allclose(_M(out[:8]), _M(a) @ _M(b), atol=1e-12)
        assert np.allclose(_M(out[8:16]), np.linalg.inv(_M(a)), atol=1e-10)
        assert np.allclose(out[16:19], (_M(a) @ np.append(p, 1))[:3], atol=1e-12)
        bse3 = b.copy(); bse3[7] = 1.0
        assert np.allclose(_M(out[19:27]), _M(a) @ _M(bse3), atol=1e-12)
        assert out[7] == pytest.approx(a[7] * b[7]) and out[15] == pytest.approx(1 / a[7]) and out[26] == pytest.approx(a[7])
