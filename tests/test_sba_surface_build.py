"""ygz::BundleAdjuster (include/ygz/Algorithm/BundleAdjuster.h, ygz_slam_amd/host/ygz_sba.cpp) and the stereo bundle adjustment's C ABI without
a device: a program written against include/ygz only compiles and links with -Wl,--no-undefined; the header declares the options, the calls
and the getters; the new C ABI symbols are bound by the loader and exported, the parameter and result blocks have one layout in the header,
the loader and the restatement; every refusal of ygz_hip_stereo_ba comes back with a null context, that is before a device is touched, each
capacity by its count alone with arrays of one element behind it."""
import ctypes
import os
import re
import subprocess

import numpy as np

import sba_ref as sb
from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/sba_surface.cpp in out_dir (also used by tests/test_gpu_sba_surface.py)"""
    exe = os.path.join(out_dir, "sba_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "sba_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_sba_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    h = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "BundleAdjuster.h")).read()
    for decl in [r"bool\s+GlobalBundleAdjustment\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*keyframes\s*\)\s*;", r"bool\s+LocalBundleAdjustment\s*\(\s*Frame\s*\*\s*keyframe\s*\)\s*;",
                 r"void\s+SetURight\s*\(\s*const\s+Frame\s*\*\s*kf\s*,\s*const\s+std::vector<double>\s*&\s*u_right\s*\)\s*;", r"void\s+ClearURight\s*\(", r"void\s+Clear\s*\(\s*\)\s*;",
                 r"double\s+_baseline\s*=\s*0\.1;", r"double\s+_chi2_mono\s*=\s*5\.991;", r"double\s+_chi2_stereo\s*=\s*7\.815;", r"int\s+_rounds\s*=\s*2;",
                 r"int\s+_robust_rounds\s*=\s*1;", r"int\s+_iterations\[4\]\s*=\s*\{\s*5,\s*10,\s*0,\s*0\s*\};", r"int\s+_gba_iterations\s*=\s*10;",
                 r"bool\s+_erase_outliers\s*=\s*true;", r"const\s+Problem\s*&\s*GetProblem\s*\(\s*\)\s*const", r"const\s+Result\s*&\s*GetResult\s*\(\s*\)\s*const",
                 r"int\s+GetOutlierCount\s*\(\s*\)\s*const"]:
        assert re.search(decl, h), decl
    assert '#include "ygz/Algorithm/BundleAdjuster.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_sba.cpp") == 2
    src = open(os.path.join(PKG, "host", "ygz_sba.cpp")).read()
    assert "BundleAdjuster::LocalBundleAdjustment" in src and "ygz_hip_stereo_ba" in src and "getenv" not in src
    lc = open(os.path.join(PKG, "host", "ygz_gba.cpp")).read()
    assert "stereo_ba" not in lc                                     # LoopClosing is not re-routed


def test_sba_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    for s in hip_lib.SBA_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    p = hip_lib.default_sba_params()
    assert (p.max_iterations, p.max_trials, p.cg_max_iterations, p.cg_batch, p.cg_tol, p.min_rel_decrease) == (10, 10, 0, 0, 1e-8, 1e-9)
    assert (p.baseline, p.chi2_mono, p.chi2_stereo, p.rounds, p.robust_rounds, list(p.iterations)) == (0.0, 5.991, 7.815, 2, 1, [5, 10, 0, 0])
    d = sb.DEFAULTS
    assert all(getattr(p, k) == d[k] for k in d if k != "iterations") and list(p.iterations) == list(d["iterations"])
    assert ctypes.sizeof(hip_lib.SbaParams) == ctypes.sizeof(sb.SbParams) == 80
    assert ctypes.sizeof(hip_lib.SbaResult) == ctypes.sizeof(sb.SbResult) == 200
    assert [(n, ctypes.sizeof(t)) for n, t in hip_lib.SbaParams._fields_] == [(n, ctypes.sizeof(t)) for n, t in sb.SbParams._fields_]
    assert [(n, ctypes.sizeof(t)) for n, t in hip_lib.SbaResult._fields_] == [(n, ctypes.sizeof(t)) for n, t in sb.SbResult._fields_]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"#define\s+YGZ_SBA_MAX_ROUNDS\s+4\b", hdr) and hip_lib.SBA_MAX_ROUNDS == sb.MAX_ROUNDS == 4
    assert re.search(r"Still 6: the stereo bundle adjustment added", hdr) and hip_lib.ABI_VERSION == 6
    # field order and sizes through a C probe: the mirrors have the header's layout
    fields_p = [n for n, _ in hip_lib.SbaParams._fields_]
    fields_r = [("lambda" if n == "lambda_" else n) for n, _ in hip_lib.SbaResult._fields_]
    src = ('#include "ygz_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void){printf("%zu %zu", sizeof(ygz_sba_params), sizeof(ygz_sba_result));\n'
           + "".join('printf(" %%zu", offsetof(ygz_sba_params, %s));\n' % n for n in fields_p)
           + "".join('printf(" %%zu", offsetof(ygz_sba_result, %s));\n' % n for n in fields_r) + "return 0;}")
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        open(os.path.join(t, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(t, "p.c"), "-o", os.path.join(t, "p")])
        got = [int(x) for x in subprocess.check_output([os.path.join(t, "p")]).split()]
    want = [80, 200] + [getattr(hip_lib.SbaParams, n).offset for n, _ in hip_lib.SbaParams._fields_] + \
           [getattr(hip_lib.SbaResult, n).offset for n, _ in hip_lib.SbaResult._fields_]
    assert got == want


def _call(hip_lib, g, null=(), N=None, L=None, E=None, K=None, **prm):
    """ygz_hip_stereo_ba with a NULL context"""
    lib = hip_lib.load()
    hip_lib.sba_argtypes(lib)
    poses, fixed, points, ep, el, obs, kind, level = sb.arrays(g)
    K = np.ascontiguousarray(g["K"] if K is None else K, np.float64)
    p = hip_lib._sba_params(**dict(dict(baseline=g.get("baseline", sb.BASELINE)), **prm))
    po, xo, res, out, chi2 = np.zeros_like(poses), np.zeros_like(points), hip_lib.SbaResult(), np.zeros(len(ep), np.uint8), np.zeros(len(ep))
    dp = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    bp = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    return lib.ygz_hip_stereo_ba(None, len(poses) if N is None else N, dp("poses", poses), bp("fixed", fixed), len(points) if L is None else L,
                                 dp("points", points), len(ep) if E is None else E, ip("edge_pose", ep), ip("edge_point", el), dp("obs", obs),
                                 bp("kind", kind), ip("level", level), dp("K4", K), ctypes.byref(p), dp("poses_out", po), dp("points_out", xo),
                                 bp("outlier", out), dp("chi2", chi2), None if "result" in null else ctypes.byref(res))


def test_every_refusal_comes_before_the_device(hip_lib):
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    g = sb.scene(3, 12, 2, seed=24)
    assert _call(hip_lib, g) == INV                                              # a valid call: only the context is missing
    for name in ["poses", "fixed", "points", "edge_pose", "edge_point", "obs", "kind", "level", "K4", "poses_out", "points_out", "result", "outlier", "chi2"]:
        assert _call(hip_lib, g, null=(name,)) == INV, name                      # outlier and chi2 may be NULL: the context is what is missing
    assert _call(hip_lib, g, N=1) == INV and _call(hip_lib, g, L=0) == INV and _call(hip_lib, g, E=0) == INV and _call(hip_lib, g, N=-1) == INV
    # capacities: the counts alone decide, with arrays of one element behind them
    one = dict(poses=np.array([[0, 0, 0, 1, 0, 0, 0.0]]), fixed=[0], points=np.zeros((1, 3)), edge_pose=[0], edge_point=[0], obs=np.zeros((1, 3)),
               kind=[1], level=[0], K=sb.K4)
    assert _call(hip_lib, one, N=hip_lib.GBA_MAX_POSES + 1, L=1, E=1) == CAP
    assert _call(hip_lib, one, N=2, L=hip_lib.GBA_MAX_POINTS + 1, E=1) == CAP
    assert _call(hip_lib, one, N=2, L=1, E=hip_lib.GBA_MAX_EDGES + 1) == CAP
    # the degree rules count present edges only
    assert _call(hip_lib, dict(g, fixed=[1, 1, 1])) == INV
    kind = np.array(g["kind"]).copy()
    kind[np.flatnonzero(g["edge_point"] == 11)[0]] = 0
    assert _call(hip_lib, dict(g, kind=kind)) == INV                             # point 11 has one present edge
    kind = np.array(g["kind"]).copy()
    kind[np.asarray(g["edge_pose"]) == 2] = 0
    assert _call(hip_lib, dict(g, kind=kind)) == INV                             # free pose 2 has no present edge
    for key, bad in [("edge_pose", 3), ("edge_pose", -1), ("edge_point", 12), ("edge_point", -1), ("kind", 3), ("kind", 255), ("level", -1), ("level", 16)]:
        a = np.array(g[key]).copy()
        a[5] = bad
        assert _call(hip_lib, dict(g, **{key: a})) == INV, (key, bad)
    for key in ["poses", "points", "obs"]:
        for bad in [np.nan, np.inf]:
            a = np.array(g[key], float).copy()
            a[1, 1] = bad
            assert _call(hip_lib, dict(g, **{key: a})) == INV, (key, bad)
    a = np.array(g["poses"], float).copy()
    a[1, :4] = 0
    assert _call(hip_lib, dict(g, poses=a)) == INV
    assert _call(hip_lib, g, K=[np.nan, 500, 320, 240]) == INV and _call(hip_lib, g, K=[0, 500, 320, 240]) == INV
    for k, vals in [("max_iterations", (0, 1001)), ("max_trials", (0, 101)), ("cg_max_iterations", (-1, 65537)), ("cg_batch", (-1, 1025)),
                    ("cg_tol", (0.0, 1.0, np.nan)), ("min_rel_decrease", (-1e-3, 1.0, np.nan)), ("baseline", (0.0, -1.0, np.nan, np.inf)),
                    ("chi2_mono", (0.0, -1.0, np.nan, np.inf)), ("chi2_stereo", (0.0, np.nan)), ("rounds", (0, 5)), ("robust_rounds", (-1, 5)),
                    ("iterations", ((0, 10), (5, 1001), (5, 0)))]:
        for v in vals:
            assert _call(hip_lib, g, **{k: v}) == INV, (k, v)
    # the stage export makes the same checks
    lib = hip_lib.load()
    poses, fixed, points, ep, el, obs, kind, level = sb.arrays(g)
    K = np.ascontiguousarray(sb.K4, np.float64)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    p = hip_lib._sba_params(baseline=0.1)
    args = lambda n: (None, n, dp(poses), bp(fixed), len(points), dp(points), len(ep), ip(ep), ip(el), dp(obs), bp(kind), ip(level), dp(K),
                      ctypes.byref(p)) + (None,) * 9
    assert lib.ygz_hip_sba_linearize(*args(len(poses))) == INV and lib.ygz_hip_sba_linearize(*args(hip_lib.GBA_MAX_POSES + 1)) == CAP
