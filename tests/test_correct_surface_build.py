"""ygz::LoopClosing::CorrectLoop (include/ygz/Algorithm/LoopClosing.h, ygz_slam_amd/host/ygz_correct.cpp) and the pose-graph C ABI without a
device: a program written against include/ygz only compiles and links with -Wl,--no-undefined; the header declares both overloads, the option
and the statistics; the new C ABI symbols are bound by the loader and exported; every refusal of ygz_hip_pose_graph_optimize comes back with a
null context, that is before a device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pgo_ref as pg
from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/correct_surface.cpp into a shared object in out_dir (also used by tests/test_gpu_loop_correct.py)"""
    so = os.path.join(out_dir, "libcorrect_surface.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "correct_surface.cpp"), "-o", so, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return so


def test_correct_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    program = ctypes.CDLL(build_program(str(tmp_path)))
    assert hasattr(program, "correct_run") and hasattr(program, "correct_blob")


def test_public_surface():
    h = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "LoopClosing.h")).read()
    for decl in [r"bool\s+CorrectLoop\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*keyframes\s*\)\s*;", r"bool\s+CorrectLoop\s*\(\s*\)\s*;",
                 r"int\s+_min_essential_weight\s*=\s*100;", r"int\s+correct_vertices\s*=\s*0;", r"int\s+correct_tree_edges\s*=\s*0;",
                 r"int\s+correct_covisibility_edges\s*=\s*0;", r"int\s+correct_loop_edges\s*=\s*0;",
                 r"vector<unsigned long>\s+correct_left_out;", r"int\s+correct_points_moved\s*=\s*0;", r"\}\s*pose_graph;",
                 r"const\s+PoseGraph\s*&\s*GetPoseGraph\s*\(\s*\)\s*const"]:
        assert re.search(decl, h), decl
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_correct.cpp") == 2
    src = open(os.path.join(PKG, "host", "ygz_correct.cpp")).read()
    assert "LoopClosing::CorrectLoop" in src and "ygz_hip_pose_graph_optimize" in src and "getenv" not in src


def test_pgo_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    for s in hip_lib.PGO_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    p = hip_lib.default_pgo_params()
    assert (p.max_iterations, p.max_trials, p.cg_max_iterations, p.fix_scale, p.cg_tol, p.min_rel_decrease) == (20, 10, 0, 0, 1e-8, 1e-9)
    assert ctypes.sizeof(hip_lib.PgoParams) == 32 and ctypes.sizeof(hip_lib.PgoResult) == 48
    assert ctypes.sizeof(pg.PgParams) == 32 and ctypes.sizeof(pg.PgResult) == 48
    assert (hip_lib.PGO_MAX_VERTICES, hip_lib.PGO_MAX_EDGES) == (4096, 32768)
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"#define\s+YGZ_PGO_MAX_VERTICES\s+4096", hdr) and re.search(r"#define\s+YGZ_PGO_MAX_EDGES\s+32768", hdr)
    # sizeof through a C probe: the mirrors have the header's layout
    src = '#include "ygz_hip.h"\n#include <stdio.h>\nint main(void){printf("%zu %zu", sizeof(ygz_pgo_params), sizeof(ygz_pgo_result));return 0;}'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        assert [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()] == [32, 48]


def _call(hip_lib, g, prm=None, S_out=True, result=True, null=()):
    """ygz_hip_pose_graph_optimize with a NULL context; `null`: the arrays passed as NULL"""
    lib = hip_lib.load()
    S, fixed, edges, M = hip_lib.pgo_arrays(g["S"], g["fixed"], g["edges"], g["M"])
    hip_lib.pgo_argtypes(lib)
    out, res = np.zeros_like(S), hip_lib.PgoResult()
    P = lambda name, a, t: None if name in null else a.ctypes.data_as(ctypes.POINTER(t))
    return lib.ygz_hip_pose_graph_optimize(None, g.get("N", len(S)), P("S", S, ctypes.c_double), P("fixed", fixed, ctypes.c_uint8),
                                           g.get("E", len(edges)), P("edges", edges, ctypes.c_int32), P("M", M, ctypes.c_double),
                                           ctypes.byref(prm) if prm is not None else None, P("S_out", out, ctypes.c_double),
                                           ctypes.byref(res) if "result" not in null else None)


def test_every_refusal_comes_before_the_device(hip_lib):
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    g = pg.ring(8, chords=2, seed=1)
    assert _call(hip_lib, g) == INV                                              # a valid graph: only the context is missing
    for name in ["S", "fixed", "edges", "M", "S_out", "result"]:
        assert _call(hip_lib, g, null=(name,)) == INV, name
    assert _call(hip_lib, dict(g, N=1)) == INV and _call(hip_lib, dict(g, E=0)) == INV
    assert _call(hip_lib, dict(g, fixed=np.ones(8, np.uint8))) == INV            # no free vertex

    def edited(key, idx, value):
        a = np.array(g[key], copy=True)
        a[idx] = value
        return dict(g, **{key: a})
    assert _call(hip_lib, edited("edges", 2, (3, 3))) == INV                     # i = j
    assert _call(hip_lib, edited("edges", 2, (3, 8))) == INV and _call(hip_lib, edited("edges", 2, (-1, 3))) == INV
    lone = dict(S=np.concatenate([g["S"], [pg.IDENTITY]]), fixed=np.concatenate([g["fixed"], [0]]), edges=g["edges"], M=g["M"])
    assert _call(hip_lib, lone) == INV                                           # a free vertex without any edge
    lone["fixed"] = np.concatenate([g["fixed"], [1]])
    assert _call(hip_lib, dict(lone, fixed=np.ones(9, np.uint8))) == INV
    for key in ["S", "M"]:
        assert _call(hip_lib, edited(key, (1, 7), 0.0)) == INV and _call(hip_lib, edited(key, (1, 7), -1.0)) == INV       # scale <= 0
        assert _call(hip_lib, edited(key, (2, 4), np.nan)) == INV and _call(hip_lib, edited(key, (2, 1), np.inf)) == INV  # non-finite
    for field, bad in [("max_iterations", 0), ("max_iterations", 1001), ("max_trials", 0), ("max_trials", 101), ("cg_max_iterations", -1),
                       ("cg_max_iterations", 65537), ("cg_tol", 0.0), ("cg_tol", 1.0), ("cg_tol", float("nan")), ("min_rel_decrease", -1e-3),
                       ("min_rel_decrease", 1.0)]:
        prm = hip_lib.default_pgo_params()
        setattr(prm, field, bad)
        assert _call(hip_lib, g, prm) == INV, (field, bad)
    # capacities: the counts alone decide, before any array is read past the graph's own size
    big = pg.ring(8, seed=1)
    assert _call(hip_lib, dict(big, N=hip_lib.PGO_MAX_VERTICES + 1)) == CAP
    assert _call(hip_lib, dict(big, E=hip_lib.PGO_MAX_EDGES + 1)) == CAP
    # the stage export refuses alike
    lib = hip_lib.load()
    S, fixed, edges, M = hip_lib.pgo_arrays(g["S"], g["fixed"], g["edges"], g["M"])
    vp = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    assert lib.ygz_hip_pgo_linearize(None, len(S), vp(S, ctypes.c_double), vp(fixed, ctypes.c_uint8), len(edges), vp(edges, ctypes.c_int32),
                                     vp(M, ctypes.c_double), None, None, None, None, None) == INV
    assert lib.ygz_hip_pgo_linearize(None, len(S), None, vp(fixed, ctypes.c_uint8), len(edges), vp(edges, ctypes.c_int32),
                                     vp(M, ctypes.c_double), None, None, None, None, None) == INV
