"""The stereo local-map surface without a device: tests/cpp/slm_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the C ABI symbols are bound by the loader, exported and declared; ygz_slm_params has the same size, field offsets and
defaults in the header and in _lib.py, and the three limits are the same; every invalid call comes back with its code and a null context (the
context is checked last, so a valid call with a null context is refused too); SCR_SLM is 43; the new sources read no environment variable;
ygz_slm.cpp calls the entry point from one place."""
import ctypes
import os
import re
import subprocess

import numpy as np

import slm_ref
from conftest import ROOT
from test_svo_surface_build import struct_from_header

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "slm.hip"), os.path.join(PKG, "csrc", "ur_dev.h"), os.path.join(PKG, "host", "ygz_slm.cpp"),
               os.path.join(ROOT, "tests", "cpp", "slm_surface.cpp"), os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoLocalMap.h"),
               os.path.join(ROOT, "tests", "slm_ref.py"), os.path.join(ROOT, "tools", "slm_bench.py")]


def build_program(out_dir):
    """compile tests/cpp/slm_surface.cpp into a program in out_dir (also used by tests/test_gpu_slm_surface.py)"""
    exe = os.path.join(out_dir, "slm_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "slm_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoLocalMap.h")).read()
    for decl in [r"int\s+TrackLocalMap\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*frames\s*,\s*const\s+std::vector<const\s+std::vector<Frame\s*\*>\s*\*>\s*&"
                 r"\s*local_keyframes\s*,\s*std::vector<Result>\s*\*\s*results\s*\)", r"struct\s+Result\b", r"creates no point and no keyframe"]:
        assert re.search(decl, hdr), decl
    opts = [("_baseline", "0.1"), ("_th", "1.0"), ("_ratio", "0.8"), ("_r_near", "2.5"), ("_r_wide", "4.0"), ("_cos_near", "0.998"),
            ("_th_dist", "100"), ("_min_edges", "3"), ("_min_tracked", "30")]
    at = -1
    for opt, val in opts:
        m = re.search(r"\b%s\s*=\s*%s\s*;" % (opt, re.escape(val)), hdr)
        assert m and m.start() > at, opt
        at = m.start()
    assert '#include "ygz/Algorithm/StereoLocalMap.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_slm.cpp") == 2
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_slm.cpp")).read())
    # one entry point, called from one place; the slots are filled by the shared loader, called from one place (test_svo_surface_build.py
    # holds the loader itself); the point set goes through the shared append; no point and no keyframe is made, and the host-array calls are
    # not used
    assert host.count("ygz_hip_stereo_local_map_slots(") == 1 and host.count("load_slots(") == 1
    assert host.count("ygz_hip_describe_given_angle(") == 0 and host.count("ygz_hip_set_keypoint_depths(") == 0 and host.count("PointAttributes(") == 0
    for word in ("Memory::", "CreateMapPoint", "RegisterKeyFrame", "ygz_hip_stereo_track_search", "ygz_hip_optimize_pose_stereo", "StereoTracker",
                 "PoseOptimizer"):
        assert word not in host, word
    others = [f for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".cpp") and f != "ygz_slm.cpp"]
    assert all("ygz_hip_stereo_local_map_slots" not in open(os.path.join(PKG, "host", f)).read() for f in others)
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code and "environ" not in code, path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.SLM_SYMBOLS == ["ygz_hip_default_slm_params", "ygz_hip_stereo_local_map_slots"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: stereo local-map tracking on resident slots added", hdr) and hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for s in hip_lib.SLM_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    for name, value, bound, ref in (("FRAMES", 1024, hip_lib.SLM_MAX_FRAMES, slm_ref.MAX_FRAMES), ("SETS", 64, hip_lib.SLM_MAX_SETS, slm_ref.MAX_SETS),
                                    ("PAIRS", 4194304, hip_lib.SLM_MAX_PAIRS, slm_ref.MAX_PAIRS)):
        assert re.search(r"#define\s+YGZ_SLM_MAX_%s\s+%d\b" % (name, value), hdr) and bound == value == ref, name
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"SCR_SLM == 43", internal) and re.search(r"SCR_SVO == 42", internal) and "SCR_STRACK, SCR_SVO, SCR_SLM," in internal
    assert re.search(r"SCR_LAST == SCR_SLM", internal) and "KID_SLM_GATHER, KID_SLM_RESOLVE, KID_SLM_SCATTER," in internal
    ctx = open(os.path.join(PKG, "csrc", "ctx.hip")).read()
    assert '"k_slm_gather", "k_slm_resolve", "k_slm_scatter",' in ctx
    # the enumerators and the names are in the same order
    ids = re.search(r"enum \{ KID_BGR2GRAY = 0,(.*?)KID_COUNT \}", internal, re.S).group(0)
    names = re.search(r"k_kernel_names\[KID_COUNT\] = \{(.*?)\};", ctx, re.S).group(1)
    assert len(re.findall(r"KID_\w+", ids)) - 1 == len(re.findall(r'"k_\w+"', names))
    assert [m.start() for m in re.finditer(r"KID_\w+", ids)].index(ids.index("KID_SLM_GATHER")) == re.findall(r'"(k_\w+)"', names).index("k_slm_gather")
    slm = open(os.path.join(PKG, "csrc", "slm.hip")).read()
    assert "ygz_blob_open(ctx, SCR_SLM" in slm


def test_struct_layout_defaults_and_limits(hip_lib, tmp_path):
    """the header's struct, compiled, against the ctypes struct: size, every offset, every default"""
    fields = struct_from_header("ygz_slm_params")
    names = ["baseline", "th", "ratio", "r_near", "r_wide", "cos_near", "th_dist", "min_edges", "pose"]
    assert [f for f, _ in fields] == [n for n, _ in hip_lib.SlmParams._fields_] == names
    pose_fields = [f for f, _ in struct_from_header("ygz_pose_opt_params")]
    assert pose_fields == [n for n, _ in hip_lib.PoseOptParams._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ygz_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d %d\\n", sizeof(ygz_slm_params), YGZ_SLM_MAX_FRAMES, YGZ_SLM_MAX_SETS, YGZ_SLM_MAX_PAIRS);']
    lines += ['  printf("%%zu\\n", offsetof(ygz_slm_params, %s));' % f for f, _ in fields]
    lines += ['  printf("%%zu\\n", offsetof(ygz_slm_params, pose.%s));' % f for f in pose_fields]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(got[0]) == ctypes.sizeof(hip_lib.SlmParams) == 112
    assert [int(v) for v in got[1:4]] == [hip_lib.SLM_MAX_FRAMES, hip_lib.SLM_MAX_SETS, hip_lib.SLM_MAX_PAIRS]
    offs = [int(v) for v in got[4:]]
    want = [getattr(hip_lib.SlmParams, n).offset for n, _ in hip_lib.SlmParams._fields_]
    want += [hip_lib.SlmParams.pose.offset + getattr(hip_lib.PoseOptParams, n).offset for n in pose_fields]
    assert offs == want
    assert re.search(r"sizeof: ygz_slm_params 112", open(os.path.join(ROOT, "include", "ygz_hip.h")).read())
    lib = hip_lib.load()
    hip_lib.slm_argtypes(lib)
    hip_lib.popt_argtypes(lib)
    p = hip_lib.SlmParams()
    p.th_dist, p.min_edges = 7, 7
    lib.ygz_hip_default_slm_params(ctypes.byref(p))
    lib.ygz_hip_default_slm_params(None)                                             # no effect, no crash
    assert (p.baseline, p.th, p.ratio, p.r_near, p.r_wide, p.cos_near, p.th_dist, p.min_edges) == (0.1, 1.0, 0.8, 2.5, 4.0, 0.998, 100, 3)
    assert {k: getattr(p, k) for k in slm_ref.DEFAULTS} == slm_ref.DEFAULTS
    q = hip_lib.PoseOptParams()
    lib.ygz_hip_default_pose_opt_params(ctypes.byref(q))
    q.baseline = 0.1
    assert bytes(p.pose) == bytes(q) and (q.rounds, q.iterations, q.max_trials, q.robust_rounds, q.min_edges, q.min_inliers) == (4, 10, 10, 3, 3, 10)


def test_every_invalid_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.slm_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    ip, dp, bp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    I = [0, 0, 0, 1.0, 0, 0, 0]

    def params(**fields):
        p = hip_lib.SlmParams()
        lib.ygz_hip_default_slm_params(ctypes.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p, k)
            getattr(tgt, name)
            setattr(tgt, name, v)
        return p

    def a_set(n=5, drop=None, n_pt=None, nan=None):
        arr = dict(pw=np.ones((n, 3)), pt_desc=np.zeros((n, 32), np.uint8), pt_dmax=np.ones(n), pt_normal=np.ones((n, 3)))
        if nan:
            arr[nan][n - 1] = np.nan
        s = hip_lib.StrackPoints()
        s.pw, s.pt_desc = arr["pw"].ctypes.data_as(dp), arr["pt_desc"].ctypes.data_as(bp)
        s.pt_dmax, s.pt_normal = arr["pt_dmax"].ctypes.data_as(dp), arr["pt_normal"].ctypes.data_as(dp)
        if drop:
            setattr(s, drop, type(getattr(s, drop))())
        s.n_pt = n if n_pt is None else n_pt
        return s, arr

    def call(sets=None, n_sets=None, slot=(0, 1), st=(0, 0), n=None, T=None, p=None, null=()):
        made = [a_set()] if sets is None else sets
        sa = (hip_lib.StrackPoints * max(len(made), 1))(*[m[0] for m in made])
        sl, se = np.array(slot, np.int32), np.array(st, np.int32)
        n = len(sl) if n is None else n
        Ta = np.ascontiguousarray(np.tile(I, (max(len(sl), 1), 1)) if T is None else T, np.float64)
        out = np.zeros((max(len(sl), 1), 7))
        arg = dict(sets=sa, slot=sl.ctypes.data_as(ip), set=se.ctypes.data_as(ip), T=Ta.ctypes.data_as(dp), out=out.ctypes.data_as(dp))
        for k in null:
            arg[k] = None
        return lib.ygz_hip_stereo_local_map_slots(None, len(made) if n_sets is None else n_sets, arg["sets"], n, arg["slot"], arg["set"], arg["T"],
                                                  None, None if p is None else ctypes.byref(p), arg["out"], *([None] * 20))
    assert call() == INV                                                         # valid: only the context is missing
    assert call(p=params()) == INV and call(sets=[a_set(0, n_pt=0)]) == INV      # a set of 0 points is a valid set
    for k in ("sets", "slot", "set", "T", "out"):
        assert call(null=(k,)) == INV, k
    assert call(n=0) == INV and call(n=-1) == INV and call(n_sets=0) == INV and call(n_sets=-1) == INV
    big = hip_lib.SLM_MAX_FRAMES + 1
    assert call(slot=[0] * big, st=[0] * big) == CAP and call(slot=[0] * (big - 1), st=[0] * (big - 1)) == INV
    assert call(slot=[0] * big, st=[0] * big, p=params(th=-1.0)) == CAP          # the counts are checked before the parameters
    one = a_set()
    assert call(sets=[one] * (hip_lib.SLM_MAX_SETS + 1)) == CAP and call(sets=[one] * hip_lib.SLM_MAX_SETS) == INV
    for bad in (dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(th=0.0), dict(th=-1.0),
                dict(th=float("nan")), dict(th=float("inf")), dict(ratio=0.0), dict(ratio=float("nan")), dict(r_near=0.0), dict(r_wide=-4.0),
                dict(r_near=float("inf")), dict(cos_near=float("nan")), dict(th_dist=-1), dict(th_dist=257), dict(min_edges=-1),
                dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=-1.0), dict(pose_chi2_mono=float("nan")), dict(pose_chi2_stereo=float("inf")),
                dict(pose_min_rel_decrease=float("nan")), dict(pose_rounds=0), dict(pose_rounds=9), dict(pose_iterations=0),
                dict(pose_iterations=65), dict(pose_max_trials=0), dict(pose_max_trials=65)):
        assert call(p=params(**bad)) == INV, bad
    assert call(sets=[a_set(n_pt=-1)]) == INV
    for drop in ("pw", "pt_desc", "pt_dmax", "pt_normal"):
        assert call(sets=[a_set(drop=drop)]) == INV, drop
    assert call(slot=(0, -1)) == INV and call(st=(0, 1)) == INV and call(st=(-1, 0)) == INV
    # more than YGZ_SLM_MAX_PAIRS pairs: 1024 frames on a set of 4097 points, and the limit itself
    assert call(sets=[a_set(4097)], slot=[0] * 1024, st=[0] * 1024) == CAP and call(sets=[a_set(4096)], slot=[0] * 1024, st=[0] * 1024) == INV
    for k in range(7):
        for bad in (np.nan, np.inf, -np.inf):
            T = np.tile(I, (2, 1))
            T[1, k] = bad
            assert call(T=T) == INV, (k, bad)
    for nan in ("pw", "pt_dmax", "pt_normal"):
        assert call(sets=[a_set(nan=nan)]) == INV, nan
