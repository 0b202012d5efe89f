"""ygz::LoopClosing::FuseLoop / UpdateCovisibility / ReplaceMapPoint, Matcher::ComputeDistinctiveDescriptors (include/ygz/Algorithm,
ygz_slam_amd/host/ygz_fuse.cpp) and the map-upkeep C ABI without a device: a program written against include/ygz only compiles and links with
-Wl,--no-undefined; the headers declare the new methods, the option and the statistics; the two C ABI symbols are bound by the loader and
exported; every refusal of ygz_hip_distinctive_descriptors and ygz_hip_covisibility comes back with a null context, that is before a device is
touched, each capacity one by its count alone."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/fuse_surface.cpp into a shared object in out_dir (also used by tests/test_gpu_loop_fuse.py)"""
    so = os.path.join(out_dir, "libfuse_surface.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "fuse_surface.cpp"), "-o", so, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return so


def test_fuse_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    program = ctypes.CDLL(build_program(str(tmp_path)))
    assert hasattr(program, "fuse_run") and hasattr(program, "fuse_blob")


def test_public_surface():
    h = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "LoopClosing.h")).read()
    for decl in [r"bool\s+FuseLoop\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*keyframes\s*\)\s*;", r"bool\s+FuseLoop\s*\(\s*\)\s*;",
                 r"static\s+void\s+ReplaceMapPoint\s*\(\s*MapPoint\s*\*\s*from\s*,\s*MapPoint\s*\*\s*into\s*\)\s*;",
                 r"int\s+UpdateCovisibility\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*rows\s*,\s*const\s+vector<Frame\s*\*>\s*&\s*keyframes\s*\)\s*;",
                 r"float\s+_fuse_search_th\s*=\s*4\.0f;", r"GetFusedPairs\s*\(\s*\)\s*const"]:
        assert re.search(decl, h), decl
    for counter in ["fuse_current_replaced", "fuse_current_added", "fuse_targets", "fuse_hits", "fuse_replaced", "fuse_added", "fuse_conflicts",
                    "fuse_descriptors", "fuse_rows"]:
        assert re.search(r"int\s+%s\s*=\s*0;" % counter, h), counter
    assert "Fusing duplicated map points, covisibility updates and a global BA are not part of it" not in h
    m = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "Matcher.h")).read()
    assert re.search(r"int\s+ComputeDistinctiveDescriptors\s*\(\s*const\s+vector<MapPoint\s*\*>\s*&\s*points\s*\)\s*;", m)
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_fuse.cpp") == 2
    src = open(os.path.join(PKG, "host", "ygz_fuse.cpp")).read()
    for name in ["LoopClosing::FuseLoop", "LoopClosing::ReplaceMapPoint", "LoopClosing::UpdateCovisibility",
                 "Matcher::ComputeDistinctiveDescriptors", "ygz_hip_distinctive_descriptors", "ygz_hip_covisibility", "SearchFuseCandidates"]:
        assert name in src, name
    assert "getenv" not in src


def test_map_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    for s in hip_lib.MAP_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    assert (hip_lib.MAP_MAX_OBS_PER_POINT, hip_lib.MAP_MAX_OBS, hip_lib.MAP_MAX_KEYFRAMES, hip_lib.COVIS_MAX_CELLS) == (256, 1048576, 4096, 4194304)
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    for name, value in [("YGZ_MAP_MAX_OBS_PER_POINT", 256), ("YGZ_MAP_MAX_OBS", 1048576), ("YGZ_MAP_MAX_KEYFRAMES", 4096),
                        ("YGZ_COVIS_MAX_CELLS", 4194304)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    assert os.path.exists(os.path.join(PKG, "csrc", "map.hip"))


def _ip(a):
    return None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _dd(hip_lib, offsets, n_points=None, desc=True, best=True, null_offsets=False):
    """ygz_hip_distinctive_descriptors with a NULL context; the descriptor array holds one row only: no refusal may read past the offsets"""
    lib = hip_lib.load()
    hip_lib.map_argtypes(lib)
    off = np.ascontiguousarray(offsets, np.int32)
    d, b = np.zeros((1, 32), np.uint8), np.zeros(max(len(off), 1), np.int32)
    return lib.ygz_hip_distinctive_descriptors(None, len(off) - 1 if n_points is None else n_points, None if null_offsets else _ip(off),
                                               d.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if desc else None, _ip(b) if best else None,
                                               None, None)


def _cv(hip_lib, offsets, kf, K, rows, n_points=None, n_rows=None, null=()):
    """ygz_hip_covisibility with a NULL context; the weights array holds one cell only"""
    lib = hip_lib.load()
    hip_lib.map_argtypes(lib)
    off, k, r, w = (np.ascontiguousarray(a, np.int32) for a in (offsets, kf, rows, [0]))
    A = lambda name, a: None if name in null else _ip(a)
    return lib.ygz_hip_covisibility(None, len(off) - 1 if n_points is None else n_points, A("offsets", off), A("kf", k), K,
                                    len(r) if n_rows is None else n_rows, A("rows", r), A("weights", w))


def test_every_refusal_comes_before_the_device(hip_lib):
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    # descriptors
    assert _dd(hip_lib, [0, 1]) == INV                                           # a valid call: only the context is missing
    assert _dd(hip_lib, [0, 1], null_offsets=True) == INV and _dd(hip_lib, [0, 1], desc=False) == INV and _dd(hip_lib, [0, 1], best=False) == INV
    assert _dd(hip_lib, [0, 1], n_points=0) == INV and _dd(hip_lib, [0, 1], n_points=-3) == INV
    assert _dd(hip_lib, [0, 1, 0]) == INV and _dd(hip_lib, [1, 1]) == INV and _dd(hip_lib, [0, -1]) == INV
    assert _dd(hip_lib, [0, hip_lib.MAP_MAX_OBS_PER_POINT]) == INV               # 256 observations on one point are served
    assert _dd(hip_lib, [0, hip_lib.MAP_MAX_OBS_PER_POINT + 1]) == CAP           # by the count alone: one descriptor row behind it
    full = np.arange(0, hip_lib.MAP_MAX_OBS + 1, hip_lib.MAP_MAX_OBS_PER_POINT)  # 4096 points of 256: exactly the capacity
    assert full[-1] == hip_lib.MAP_MAX_OBS and _dd(hip_lib, full) == INV
    assert _dd(hip_lib, np.append(full, hip_lib.MAP_MAX_OBS + 1)) == CAP
    # weights
    ok = dict(offsets=[0, 2, 3], kf=[0, 2, 1], K=3, rows=[2, 0])
    call = lambda **kw: _cv(hip_lib, **dict(ok, **kw))
    assert call() == INV                                                         # a valid call: only the context is missing
    for name in ["offsets", "kf", "rows", "weights"]:
        assert call(null=(name,)) == INV, name
    assert call(n_points=0) == INV and call(K=0) == INV and call(n_rows=0) == INV
    assert call(kf=[0, 3, 1]) == INV and call(kf=[-1, 2, 1]) == INV              # an index out of range
    assert call(kf=[2, 0, 1]) == INV and call(kf=[2, 2, 1]) == INV               # a list that is not strictly ascending
    assert call(rows=[2, 2]) == INV and call(rows=[3]) == INV and call(rows=[-1]) == INV
    assert call(offsets=[0, 3, 2]) == INV and call(offsets=[1, 2, 3]) == INV
    # capacities: the counts alone decide, before any array is read past the case's own size
    assert call(K=hip_lib.MAP_MAX_KEYFRAMES + 1) == CAP
    assert call(K=hip_lib.MAP_MAX_KEYFRAMES, n_rows=hip_lib.COVIS_MAX_CELLS // hip_lib.MAP_MAX_KEYFRAMES + 1) == CAP
    assert call(K=3, n_rows=hip_lib.COVIS_MAX_CELLS // 3 + 1) == CAP
    assert call(offsets=[0, hip_lib.MAP_MAX_OBS + 1], kf=[0]) == CAP
