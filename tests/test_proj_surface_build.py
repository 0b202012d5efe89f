"""The projection-guided searches' class surface (include/ygz/Algorithm/Matcher.h, LoopClosing.h, ygz/Basic/Sim3.h; libygz_host.so) and their C
ABI without a device: a program written against include/ygz only (tests/cpp/proj_surface.cpp) compiles and links with -Wl,--no-undefined; the
public surface and its defaults are as declared; the new C ABI symbols are bound by the loader and the structures have the header's layout;
bad arguments are refused before a device is touched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/proj_surface.cpp into a shared object in out_dir (also used by tests/test_gpu_loop_widen.py)"""
    so = os.path.join(out_dir, "libproj_surface.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "proj_surface.cpp"), "-o", so, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return so


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    return ctypes.CDLL(build_program(str(tmp_path_factory.mktemp("proj"))))


def test_program_compiles_and_links(program):
    assert hasattr(program, "widen_run") and hasattr(program, "widen_blob")


def _has(text, decls):
    for d in decls:
        assert re.search(d, text), d


def test_public_surface():
    inc = os.path.join(ROOT, "include", "ygz")
    m = open(os.path.join(inc, "Algorithm", "Matcher.h")).read()
    _has(m, [r'#include "ygz/Basic/Sim3\.h"',
             r"int\s+SearchByProjection\s*\(\s*Frame\s*\*\s*kf\s*,\s*const\s+Sim3\s*&\s*Scw\s*,\s*const\s+vector<MapPoint\s*\*>\s*&\s*points\s*,\s*"
             r"vector<MapPoint\s*\*>\s*&\s*matched\s*,\s*float\s+th\s*\)",
             r"int\s+SearchBySim3\s*\(\s*Frame\s*\*\s*kf1\s*,\s*Frame\s*\*\s*kf2\s*,\s*vector<MapPoint\s*\*>\s*&\s*matches12\s*,\s*const\s+Sim3\s*&\s*S12\s*,"
             r"\s*float\s+th\s*\)",
             r"int\s+SearchFuseCandidates\s*\(\s*const\s+vector<Frame\s*\*>\s*&\s*kfs\s*,\s*const\s+vector<Sim3>\s*&\s*Scw\s*,\s*const\s+"
             r"vector<MapPoint\s*\*>\s*&\s*points\s*,\s*float\s+th\s*,\s*vector<vector<int>>\s*&\s*feature_of_point\s*\)",
             r"static\s+bool\s+PointAttributes\s*\("])
    s = open(os.path.join(inc, "Basic", "Sim3.h")).read()
    _has(s, [r"struct\s+Sim3\b", r"Sim3\s+inverse\s*\(\s*\)\s*const", r"void\s+to8\s*\(", r"static\s+Sim3\s+from8\s*\("])
    lc = open(os.path.join(inc, "Algorithm", "LoopClosing.h")).read()
    assert len(re.findall(r"^struct\s+Sim3\b", lc, re.M)) == 0 and '#include "ygz/Basic/Sim3.h"' in lc        # one definition, in Sim3.h
    _has(lc, [r"bool\s+SearchLoopMapPoints\s*\(\s*\)", r"int\s+_min_total_matches\s*=\s*40;",
              r"const\s+vector<MapPoint\s*\*>\s*&\s*GetCurrentMatchedPoints\s*\(\s*\)\s*const",
              r"const\s+vector<MapPoint\s*\*>\s*&\s*GetLoopMapPoints\s*\(\s*\)\s*const", r"int\s+sim3_added\b", r"int\s+projection_added\b",
              r"int\s+total_matches\b", r"bool\s+ComputeSim3\s*\(\s*\)", r"bool\s+DetectLoop\s*\(\s*Frame\s*\*\s*kf\s*\)"])
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_proj.cpp") == 2


def test_header_declares_the_abi():
    h = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    _has(h, [r"#define\s+YGZ_HIP_ABI_VERSION\s+6\b", r"Still 6: the projection-guided descriptor search added", r"#define\s+YGZ_PROJ_MAX_PROBLEMS\s+64\b",
             r"#define\s+YGZ_PROJ_TOPK\s+8\b", r"\}\s*ygz_proj_problem;", r"\}\s*ygz_proj_params;", r"void\s+ygz_hip_default_proj_params\s*\(",
             r"int\s+ygz_hip_search_by_projection\s*\(", r"int\s+ygz_hip_projection_candidates\s*\("])


def test_proj_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert lib.ygz_hip_abi_version() == 6
    for s in hip_lib.PROJ_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    p = hip_lib.default_proj_params()
    assert (p.th, p.th_dist, p.claim) == (10.0, 50, 1)
    assert ctypes.sizeof(hip_lib.ProjProblem) == 152 and ctypes.sizeof(hip_lib.ProjParams) == 16
    assert hip_lib.ProjProblem.S.offset == 88 and hip_lib.ProjProblem.n_pt.offset == 80 and hip_lib.ProjProblem.n_kp.offset == 32
    assert (hip_lib.PROJ_MAX_PROBLEMS, hip_lib.PROJ_TOPK, hip_lib.PROJ_MAX_POINTS) == (64, 8, 65536)


def test_entry_points_refuse_bad_arguments_without_device(hip_lib):
    lib = hip_lib.load()
    sc = dict(kp_px=np.zeros((4, 2)), kp_level=np.zeros(4, np.int32), kp_desc=np.zeros((4, 32), np.uint8), pw=np.ones((3, 3)),
              pt_desc=np.zeros((3, 32), np.uint8), pt_dmax=np.ones(3), S=[0, 0, 0, 1, 0, 0, 0, 1.0])
    arr, keep = hip_lib.proj_problems([sc])
    K = (ctypes.c_double * 4)(500, 500, 320, 240)
    lib.ygz_hip_search_by_projection.argtypes = None
    assert lib.ygz_hip_search_by_projection(None, 1, arr, K, None, None, None, None, None) == hip_lib.E_INVALID
    lib.ygz_hip_projection_candidates.argtypes = None
    assert lib.ygz_hip_projection_candidates(None, arr, K, None, None, None, None, None) == hip_lib.E_INVALID
    lib.ygz_hip_default_proj_params(None)                                # a null pointer is ignored
    with pytest.raises(ValueError):
        hip_lib.proj_problems([dict(sc, kp_level=np.zeros(5, np.int32))])
