"""ygz::KeyFrameCulling (include/ygz/Algorithm/KeyFrameCulling.h, ygz_slam_amd/host/ygz_cull.cpp) and the keyframe-culling C ABI without a
device: a program written against include/ygz only compiles and links with -Wl,--no-undefined; the header declares the methods, the options
and the counters; the C ABI symbols are bound by the loader and exported and the constants agree with the header; every refusal of
ygz_hip_keyframe_redundancy and ygz_hip_cull_keyframes comes back with a null context, that is before a device is touched, each capacity by
its count alone, with arrays no larger than the case needs."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/cull_surface.cpp into a shared object in out_dir (also used by tests/test_gpu_cull_surface.py)"""
    so = os.path.join(out_dir, "libcull_surface.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cull_surface.cpp"), "-o", so, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return so


def test_cull_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    program = ctypes.CDLL(build_program(str(tmp_path)))
    assert hasattr(program, "cull_run")


def test_public_surface():
    h = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "KeyFrameCulling.h")).read()
    for decl in [r"class\s+KeyFrameCulling\b", r"void\s+SetKeyFrameDatabase\s*\(\s*KeyFrameDatabase\s*\*",
                 r"void\s+SetProtected\s*\(\s*const\s+vector<Frame\s*\*>\s*&",
                 r"bool\s+Redundancy\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*kfs\s*,\s*vector<Entry>\s*&\s*out\s*\)\s*;",
                 r"int\s+Cull\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*candidates\s*,\s*vector<Frame\s*\*>\s*\*\s*culled\s*=\s*nullptr\s*\)\s*;",
                 r"static\s+void\s+SetBadFlag\s*\(\s*Frame\s*\*\s*kf\s*,\s*int\s+min_obs\s*\)\s*;",
                 r"struct\s+Entry\s*\{\s*Frame\s*\*kf;\s*int\s+tracked,\s*redundant;\s*\}",
                 r"int\s+th_obs\s*=\s*3;", r"double\s+ratio\s*=\s*0\.9;", r"int\s+level_slack\s*=\s*-1;", r"int\s+min_obs\s*=\s*2;",
                 r"size_t\s+min_keyframes\s*=\s*5;", r"UpdateCovisibility"]:
        assert re.search(decl, h), decl
    stats = h[h.index("struct Stats"):h.index("struct Entry")]
    for counter in ["candidates", "skipped", "universe", "points", "observations", "culled", "points_killed", "db_erased", "dead_mismatch"]:
        assert re.search(r"\b%s\s*=\s*0\b" % counter, stats), counter
    assert '#include "ygz/Algorithm/KeyFrameCulling.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_cull.cpp") == 2
    src = open(os.path.join(PKG, "host", "ygz_cull.cpp")).read()
    for name in ["KeyFrameCulling::Redundancy", "KeyFrameCulling::Cull", "KeyFrameCulling::SetBadFlag", "KeyFrameCulling::SetProtected",
                 "ygz_hip_keyframe_redundancy", "ygz_hip_cull_keyframes"]:
        assert name in src, name
    assert "getenv" not in src and "getenv" not in open(os.path.join(PKG, "csrc", "cull.hip")).read()


def test_cull_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.CULL_SYMBOLS == ["ygz_hip_default_cull_params", "ygz_hip_keyframe_redundancy", "ygz_hip_cull_keyframes"]
    for s in hip_lib.CULL_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert hip_lib.CULL_MAX_KEYFRAMES == 4096 == hip_lib.MAP_MAX_KEYFRAMES
    for name, value in [("YGZ_CULL_MAX_KEYFRAMES", 4096), ("YGZ_MAP_MAX_OBS_PER_POINT", 256), ("YGZ_MAP_MAX_OBS", 1048576)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    assert re.search(r"Still 6: keyframe culling added", hdr) and hip_lib.ABI_VERSION == 6
    # the defaults of the header's table, and the struct the restatement reads has the same layout
    p = hip_lib.default_cull_params()
    assert (p.th_obs, p.ratio, p.level_slack, p.min_obs) == (3, 0.9, -1, 2)
    import cull_ref
    assert ctypes.sizeof(hip_lib.CullParams) == ctypes.sizeof(cull_ref.Params) == 24
    assert [(n, t) for n, t in hip_lib.CullParams._fields_] == [(n, t) for n, t in cull_ref.Params._fields_]
    assert os.path.exists(os.path.join(PKG, "csrc", "cull.hip"))


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


OK_CASE = dict(offsets=[0, 2, 3], kf=[0, 2, 1], level=[0, 15, 3], K=3, cand=[2, 0])


def _call(hip_lib, walk, offsets, kf, level, K, cand, n_points=None, n_cand=None, null=(), **prm):
    """one of the two entry points with a NULL context; the outputs hold two elements only"""
    lib = hip_lib.load()
    hip_lib.cull_argtypes(lib)
    off = np.ascontiguousarray(offsets, np.int32)
    out = [np.zeros(2, np.int32) for _ in range(3)]
    A = lambda name, a: None if name in null else _ip(a)
    q = None if prm.pop("no_params", False) else ctypes.byref(hip_lib._cull_params(**prm))
    P = len(off) - 1 if n_points is None else n_points
    if not walk:
        return lib.ygz_hip_keyframe_redundancy(None, P, A("offsets", off), A("kf", kf), A("level", level), K, q, A("tracked", out[1]),
                                               A("redundant", out[2]))
    return lib.ygz_hip_cull_keyframes(None, P, A("offsets", off), A("kf", kf), A("level", level), K, len(cand) if n_cand is None else n_cand,
                                      A("cand", cand), q, A("culled", out[0]), A("tracked", out[1]), A("redundant", out[2]), None)


def test_every_refusal_comes_before_the_device(hip_lib):
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    CK, OBS, PER = hip_lib.CULL_MAX_KEYFRAMES, hip_lib.MAP_MAX_OBS, hip_lib.MAP_MAX_OBS_PER_POINT
    for walk in (False, True):
        call = lambda **kw: _call(hip_lib, walk, **dict(OK_CASE, **kw))
        assert call() == INV and call(no_params=True) == INV                     # a valid call: only the context is missing
        nulls = ["offsets", "kf", "level", "tracked", "redundant"] + (["cand", "culled"] if walk else [])
        for name in nulls:
            assert call(null=(name,)) == INV, name
            assert call(null=(name,), K=CK + 1) == INV, name                     # a null array comes first
        assert call(n_points=0) == INV and call(n_points=-2) == INV and call(K=0) == INV and call(K=-1) == INV
        assert call(offsets=[1, 2, 3]) == INV and call(offsets=[0, 3, 2]) == INV
        assert call(kf=[0, 3, 1]) == INV and call(kf=[-1, 2, 1]) == INV          # an index out of range
        assert call(kf=[2, 0, 1]) == INV and call(kf=[2, 2, 1]) == INV           # a list that is not strictly ascending
        assert call(level=[0, 16, 3]) == INV and call(level=[0, 15, -1]) == INV
        assert call(level=[15, 0, 15]) == INV                                    # the levels' edge is valid
        for bad in [dict(th_obs=0), dict(th_obs=257), dict(min_obs=-1), dict(min_obs=257), dict(level_slack=-2), dict(level_slack=16),
                    dict(ratio=-0.01), dict(ratio=1.01), dict(ratio=float("nan")), dict(ratio=float("inf"))]:
            assert call(**bad) == INV, bad
        for edge in [dict(th_obs=1), dict(th_obs=256), dict(min_obs=0), dict(min_obs=256), dict(level_slack=15), dict(ratio=0.0), dict(ratio=1.0)]:
            assert call(**edge) == INV, edge                                     # valid: only the context is missing
        # capacities: the counts alone decide, before any array is read past the case's own size
        assert call(K=CK + 1) == CAP and call(K=CK + 1, kf=[9999, -5, 0], th_obs=0) == CAP
        assert call(K=CK) == INV
        assert call(offsets=[0, PER], kf=np.arange(PER), level=np.zeros(PER), K=PER, cand=[5]) == INV   # 256 observations on one point are served
        assert call(offsets=[0, PER + 1], kf=[0], level=[0]) == CAP              # one element behind each array
        full = np.arange(0, OBS + 1, PER)                                        # 4096 points of 256: exactly the capacity
        assert full[-1] == OBS
        assert call(offsets=np.append(full, OBS + 1), kf=[0], level=[0]) == CAP
    walk = lambda **kw: _call(hip_lib, True, **dict(OK_CASE, **kw))
    assert walk(cand=[0], n_cand=0) == INV and walk(cand=[0], n_cand=-1) == INV
    assert walk(cand=[2, 2]) == INV and walk(cand=[3]) == INV and walk(cand=[-1]) == INV
    assert walk(cand=[0], n_cand=CK + 1) == CAP and walk(cand=[7, 7], n_cand=CK + 1, K=0) == CAP
    assert walk(cand=[1, 0, 2]) == INV                                           # every keyframe a candidate: valid
