"""The stereo pose optimisation's surface without a device: tests/cpp/popt_surface.cpp, written against include/ygz only, compiles and links
with -Wl,--no-undefined; PoseOptimizer is declared and listed in Algorithm.h; the C ABI symbols are bound by the loader and exported; every
invalid call comes back YGZ_E_INVALID with a null context (the context is checked last, so a valid call with a null context is refused too);
ygz_pose_opt_params has the size, the fields and the defaults of the restatement's struct (but the baseline, which has no default) and the
status codes agree; the new sources read no environment variable."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import popt_ref as pr

PKG = os.path.join(ROOT, "ygz_slam_amd")
FIELDS = ["baseline", "chi2_mono", "chi2_stereo", "rounds", "iterations", "max_trials", "robust_rounds", "min_edges", "min_inliers", "min_rel_decrease"]


def build_program(out_dir):
    """compile tests/cpp/popt_surface.cpp into a program in out_dir (also used by tests/test_popt_ref.py and tests/test_gpu_popt_surface.py)"""
    exe = os.path.join(out_dir, "popt_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "popt_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "PoseOptimizer.h")).read()
    for decl in [r"class\s+PoseOptimizer", r"double\s+_baseline\s*=\s*0\.1;", r"double\s+_chi2_mono\s*=\s*5\.991;", r"double\s+_chi2_stereo\s*=\s*7\.815;",
                 r"int\s+_rounds\s*=\s*4;", r"int\s+_iterations\s*=\s*10;", r"int\s+_max_trials\s*=\s*10;", r"int\s+_robust_rounds\s*=\s*3;",
                 r"int\s+_min_edges\s*=\s*3;", r"int\s+_min_inliers\s*=\s*10;", r"double\s+_min_rel_decrease\s*=\s*0;", r"\}\s*_options;",
                 r"int\s+Optimize\s*\(\s*Frame\s*\*\s*current\s*,\s*const\s+std::vector<double>\s*\*\s*u_right\s*=\s*nullptr\s*\)",
                 r"void\s+OptimizeBatch\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*frames\s*,\s*const\s+std::vector<const\s+std::vector<double>\s*\*>\s*&\s*u_right\s*\)",
                 r"static\s+int\s+URightFromDepth\s*\(\s*const\s+Frame\s*\*\s*frame\s*,\s*double\s+baseline\s*,\s*std::vector<double>\s*\*\s*u_right\s*\)",
                 r"GetOutliers\(\)", r"GetRounds\(\)", r"GetInliers\(\)"]:
        assert re.search(decl, hdr), decl
    assert '#include "ygz/Algorithm/PoseOptimizer.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_popt.cpp") == 2
    host = open(os.path.join(PKG, "host", "ygz_popt.cpp")).read()
    assert host.count("ygz_hip_optimize_pose_stereo(") == 1                          # one call for all frames of a batch
    for path in (os.path.join(PKG, "host", "ygz_popt.cpp"), os.path.join(PKG, "csrc", "popt.hip"), os.path.join(PKG, "csrc", "posemath_dev.h"),
                 os.path.join(ROOT, "tests", "cpp", "popt_surface.cpp")):
        assert "getenv" not in open(path).read(), path
    # Feature keeps its layout: the surface adds no member to it
    feat = open(os.path.join(ROOT, "include", "ygz", "Basic", "Feature.h")).read()
    assert "u_right" not in feat and "_uright" not in feat


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.POPT_SYMBOLS == ["ygz_hip_default_pose_opt_params", "ygz_hip_optimize_pose_stereo"]
    for s in hip_lib.POPT_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: stereo pose optimisation added", hdr) and hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for s in hip_lib.POPT_SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    body = re.search(r"typedef struct \{([^}]*)\} ygz_pose_opt_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(double|int)\s+", "", decl.strip()).split(",")]
    assert names == FIELDS == [n for n, _ in hip_lib.PoseOptParams._fields_] == [n for n, _ in pr.Params._fields_]
    assert ctypes.sizeof(hip_lib.PoseOptParams) == ctypes.sizeof(pr.Params) == pr.lib().pr_params_size() == 56
    for (n, t), (rn, rtype) in zip(hip_lib.PoseOptParams._fields_, pr.Params._fields_):
        assert getattr(hip_lib.PoseOptParams, n).offset == getattr(pr.Params, rn).offset and ctypes.sizeof(t) == ctypes.sizeof(rtype), n
    # the status codes: the header, the loader, the restatement
    for v, name in enumerate(["FAILED", "CONVERGED", "MAX_ITERATIONS", "STALLED"]):
        assert re.search(r"#define\s+YGZ_POPT_%s\s+%d\b" % (name, v), hdr), name
        assert getattr(hip_lib, "POPT_" + name) == getattr(pr, name) == v
    assert re.search(r"#define\s+YGZ_POPT_MAX_ROUNDS\s+8\b", hdr) and hip_lib.POPT_MAX_ROUNDS == pr.MAX_ROUNDS == 8
    assert re.search(r"#define\s+YGZ_POPT_MAX_STEPS\s+64\b", hdr) and hip_lib.POPT_MAX_STEPS == 64
    ref = open(os.path.join(ROOT, "tests", "popt_ref.c")).read()
    assert re.search(r"enum \{ PR_FAILED = 0, PR_CONVERGED = 1, PR_MAX_ITERATIONS = 2, PR_STALLED = 3 \}", ref) and "#define PR_MAX_ROUNDS 8" in ref
    # the defaults
    hip_lib.popt_argtypes(lib)
    p = hip_lib.PoseOptParams(9.0, 9.0, 9.0, 9, 9, 9, 9, 9, 9, 9.0)
    lib.ygz_hip_default_pose_opt_params(ctypes.byref(p))
    q = pr.Params()
    pr.lib().pr_default_params(ctypes.byref(q))
    assert tuple(getattr(p, n) for n in FIELDS) == (0.0, 5.991, 7.815, 4, 10, 10, 3, 3, 10, 0.0) == tuple(pr.fields(q).values())
    lib.ygz_hip_default_pose_opt_params(None)


def test_every_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.popt_argtypes(lib)
    INV = hip_lib.E_INVALID
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    off, pw, obs = np.array([0, 2, 4], np.int32), np.ones((4, 3)), np.ones((4, 3))
    level, kind, poses = np.zeros(4, np.int32), np.array([1, 2, 0, 1], np.uint8), np.tile([0, 0, 0, 1.0, 0, 0, 0], (2, 1))

    def prm(**kw):
        v = dict(zip(FIELDS, (0.1, 5.991, 7.815, 4, 10, 10, 3, 3, 10, 0.0)))
        v.update(kw)
        return hip_lib.PoseOptParams(*[v[n] for n in FIELDS])

    def call(p, n_frames=2, off=off, kind=kind):
        before = poses.copy()
        rc = lib.ygz_hip_optimize_pose_stereo(None, n_frames, ip(off), dp(pw), dp(obs), ip(level), bp(kind), p, dp(poses), *(None,) * 9)
        assert np.array_equal(before, poses)
        return rc
    assert call(ctypes.byref(prm())) == INV                                         # valid: only the context is missing
    assert call(ctypes.byref(prm()), n_frames=0) == INV
    assert call(None) == INV
    assert call(ctypes.byref(prm()), n_frames=-1) == INV
    assert call(ctypes.byref(prm()), off=np.array([1, 2, 4], np.int32)) == INV
    assert call(ctypes.byref(prm()), off=np.array([0, 3, 2], np.int32)) == INV
    assert call(ctypes.byref(prm()), kind=np.array([1, 3, 0, 1], np.uint8)) == INV
    nan, inf = float("nan"), float("inf")
    for bad in (dict(baseline=0.0), dict(baseline=-1.0), dict(baseline=nan), dict(baseline=inf), dict(chi2_mono=0.0), dict(chi2_mono=nan),
                dict(chi2_stereo=-2.0), dict(chi2_stereo=inf), dict(min_rel_decrease=nan), dict(rounds=0), dict(rounds=9), dict(iterations=0),
                dict(iterations=65), dict(max_trials=0), dict(max_trials=65)):
        assert call(ctypes.byref(prm(**bad))) == INV, bad
