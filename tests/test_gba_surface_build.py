"""ygz::LoopClosing::GlobalBundleAdjustment (include/ygz/Algorithm/LoopClosing.h, ygz_slam_amd/host/ygz_gba.cpp) and the global-BA C ABI
without a device: a program written against include/ygz only compiles and links with -Wl,--no-undefined; the header declares both overloads,
the options, the statistics and the getter; the new C ABI symbols are bound by the loader and exported; every refusal of ygz_hip_global_ba
comes back with a null context, that is before a device is touched, each capacity by its count alone with arrays of one element behind it."""
import ctypes
import os
import re
import subprocess

import numpy as np

import gba_ref as gb
from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/gba_surface.cpp into a shared object in out_dir (also used by tests/test_gpu_loop_gba.py)"""
    so = os.path.join(out_dir, "libgba_surface.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gba_surface.cpp"), "-o", so, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return so


def test_gba_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    program = ctypes.CDLL(build_program(str(tmp_path)))
    assert hasattr(program, "gba_run") and hasattr(program, "gba_blob")


def test_public_surface():
    h = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "LoopClosing.h")).read()
    for decl in [r"bool\s+GlobalBundleAdjustment\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*keyframes\s*\)\s*;", r"bool\s+GlobalBundleAdjustment\s*\(\s*\)\s*;",
                 r"int\s+_gba_iterations\s*=\s*10;", r"double\s+_gba_huber_delta\s*=\s*5\.991;", r"int\s+gba_poses\s*=\s*0;", r"int\s+gba_points\s*=\s*0;",
                 r"int\s+gba_edges\s*=\s*0;", r"int\s+gba_points_left_out\s*=\s*0;", r"\}\s*global_ba;",
                 r"const\s+BundleProblem\s*&\s*GetBundleProblem\s*\(\s*\)\s*const"]:
        assert re.search(decl, h), decl
    assert "no global BA follows" not in h and "not including, the global BA" not in h
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_gba.cpp") == 2
    src = open(os.path.join(PKG, "host", "ygz_gba.cpp")).read()
    assert "LoopClosing::GlobalBundleAdjustment" in src and "ygz_hip_global_ba" in src and "getenv" not in src


def test_gba_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    for s in hip_lib.GBA_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    p = hip_lib.default_gba_params()
    assert (p.max_iterations, p.max_trials, p.cg_max_iterations, p.cg_batch, p.cg_tol, p.min_rel_decrease) == (10, 10, 0, 0, 1e-8, 1e-9)
    assert ctypes.sizeof(hip_lib.GbaParams) == 32 and ctypes.sizeof(hip_lib.GbaResult) == 48
    assert ctypes.sizeof(gb.GbParams) == 32 and ctypes.sizeof(gb.GbResult) == 48
    assert (hip_lib.GBA_MAX_POSES, hip_lib.GBA_MAX_POINTS, hip_lib.GBA_MAX_EDGES) == (4096, 1048576, 4194304)
    assert (hip_lib.GBA_FAILED, hip_lib.GBA_CONVERGED, hip_lib.GBA_MAX_ITERATIONS, hip_lib.GBA_STALLED) == \
        (hip_lib.PGO_FAILED, hip_lib.PGO_CONVERGED, hip_lib.PGO_MAX_ITERATIONS, hip_lib.PGO_STALLED)
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    for name, value in [("YGZ_GBA_MAX_POSES", 4096), ("YGZ_GBA_MAX_POINTS", 1048576), ("YGZ_GBA_MAX_EDGES", 4194304)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    assert re.search(r"Still 6: the global bundle adjustment added", hdr)
    # sizeof through a C probe: the mirrors have the header's layout
    src = '#include "ygz_hip.h"\n#include <stdio.h>\nint main(void){printf("%zu %zu", sizeof(ygz_gba_params), sizeof(ygz_gba_result));return 0;}'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "p.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")])
        assert subprocess.check_output([os.path.join(d, "p")]).decode().split() == ["32", "48"]


def _call(hip_lib, g, null=(), N=None, L=None, E=None, K=None, huber=None, out=True, **prm):
    """ygz_hip_global_ba with a NULL context"""
    lib = hip_lib.load()
    hip_lib.gba_argtypes(lib)
    poses, fixed, points, ep, el, obs = gb.arrays(g)
    K = np.ascontiguousarray(g["K"] if K is None else K, np.float64)
    p = hip_lib.default_gba_params()
    for k, v in prm.items():
        setattr(p, k, v)
    po, xo, res = np.zeros_like(poses), np.zeros_like(points), hip_lib.GbaResult()
    dp = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    return lib.ygz_hip_global_ba(None, len(poses) if N is None else N, dp("poses", poses),
                                 None if "fixed" in null else fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                 len(points) if L is None else L, dp("points", points), len(ep) if E is None else E, ip("edge_pose", ep),
                                 ip("edge_point", el), dp("obs", obs), dp("K4", K), g["huber"] if huber is None else huber, ctypes.byref(p),
                                 dp("poses_out", po), dp("points_out", xo), None if "result" in null else ctypes.byref(res))


def test_every_refusal_comes_before_the_device(hip_lib):
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    g = gb.scene(3, 12, 2, seed=24)
    assert _call(hip_lib, g) == INV                                              # a valid call: only the context is missing
    for name in ["poses", "fixed", "points", "edge_pose", "edge_point", "obs", "K4", "poses_out", "points_out", "result"]:
        assert _call(hip_lib, g, null=(name,)) == INV, name
    assert _call(hip_lib, g, N=1) == INV and _call(hip_lib, g, L=0) == INV and _call(hip_lib, g, E=0) == INV and _call(hip_lib, g, N=-1) == INV
    # capacities: the counts alone decide, with arrays of one element behind them
    one = dict(poses=np.array([[0, 0, 0, 1, 0, 0, 0.0]]), fixed=[0], points=np.zeros((1, 3)), edge_pose=[0], edge_point=[0], obs=np.zeros((1, 2)),
               K=gb.K4, huber=gb.HUBER)
    assert _call(hip_lib, one, N=hip_lib.GBA_MAX_POSES + 1, L=1, E=1) == CAP
    assert _call(hip_lib, one, N=2, L=hip_lib.GBA_MAX_POINTS + 1, E=1) == CAP
    assert _call(hip_lib, one, N=2, L=1, E=hip_lib.GBA_MAX_EDGES + 1) == CAP
    # no free pose; a free pose without an edge; a point with fewer than two edges
    assert _call(hip_lib, dict(g, fixed=[1, 1, 1])) == INV
    lonely = dict(g, edge_pose=np.where(np.asarray(g["edge_pose"]) == 2, 1, g["edge_pose"]))
    assert _call(hip_lib, lonely) == INV and _call(hip_lib, dict(lonely, fixed=[0, 0, 1])) == INV      # fixed, the pose needs no edge
    el = np.array(g["edge_point"]).copy()
    el[el == 11] = 10
    assert _call(hip_lib, dict(g, edge_point=el)) == INV                         # point 11 has no edge
    el = np.array(g["edge_point"]).copy()
    el[np.flatnonzero(el == 11)[0]] = 10
    assert _call(hip_lib, dict(g, edge_point=el)) == INV                         # point 11 has one edge
    # an index out of range
    for key, bad in [("edge_pose", 3), ("edge_pose", -1), ("edge_point", 12), ("edge_point", -1)]:
        a = np.array(g[key]).copy()
        a[5] = bad
        assert _call(hip_lib, dict(g, **{key: a})) == INV, (key, bad)
    # a non-finite value, a zero quaternion
    for key in ["poses", "points", "obs"]:
        for bad in [np.nan, np.inf]:
            a = np.array(g[key], float).copy()
            a[1, 1] = bad
            assert _call(hip_lib, dict(g, **{key: a})) == INV, (key, bad)
    a = np.array(g["poses"], float).copy()
    a[1, :4] = 0
    assert _call(hip_lib, dict(g, poses=a)) == INV
    assert _call(hip_lib, g, K=[np.nan, 500, 320, 240]) == INV and _call(hip_lib, g, K=[0, 500, 320, 240]) == INV
    assert _call(hip_lib, g, K=[500, -1, 320, 240]) == INV and _call(hip_lib, g, huber=np.nan) == INV and _call(hip_lib, g, huber=np.inf) == INV
    assert _call(hip_lib, g, huber=0.0) == INV and _call(hip_lib, g, huber=-1.0) == INV                 # no kernel: valid, only the context is missing
    # a parameter out of its range
    for k, vals in [("max_iterations", (0, 1001)), ("max_trials", (0, 101)), ("cg_max_iterations", (-1, 65537)), ("cg_batch", (-1, 1025)),
                    ("cg_tol", (0.0, 1.0, np.nan)), ("min_rel_decrease", (-1e-3, 1.0, np.nan))]:
        for v in vals:
            assert _call(hip_lib, g, **{k: v}) == INV, (k, v)
    # the stage export makes the same checks
    lib = hip_lib.load()
    poses, fixed, points, ep, el, obs = gb.arrays(g)
    K = np.ascontiguousarray(gb.K4, np.float64)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    args = lambda n: (None, n, dp(poses), fixed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(points), dp(points), len(ep), ip(ep), ip(el),
                      dp(obs), dp(K), gb.HUBER, None) + (None,) * 9
    assert lib.ygz_hip_gba_linearize(*args(len(poses))) == INV and lib.ygz_hip_gba_linearize(*args(hip_lib.GBA_MAX_POSES + 1)) == CAP
