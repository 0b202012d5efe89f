"""The stereo tracking surface without a device: tests/cpp/strack_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the C ABI symbols are bound by the loader, exported and declared; the limits are equal in the header, in _lib.py and in the
restatement; ygz_strack_params, ygz_strack_points and ygz_strack_problem have the size and the field offsets of the restatement's structs; the
defaults are the stated ones; every invalid call comes back with its code and a null context (the context is checked last, so a valid call
with a null context is refused too); the new sources read no environment variable; ygz_strack.cpp calls the entry point from one place."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import strack_ref as st

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "strack.hip"), os.path.join(PKG, "host", "ygz_strack.cpp"), os.path.join(ROOT, "tests", "cpp", "strack_surface.cpp"),
               os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoTracker.h"), os.path.join(ROOT, "tests", "strack_ref.c")]


def build_program(out_dir):
    """compile tests/cpp/strack_surface.cpp into a program in out_dir (also used by tests/test_gpu_strack_surface.py)"""
    exe = os.path.join(out_dir, "strack_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "strack_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoTracker.h")).read()
    for decl in [r"int\s+TrackWithMotionModel\s*\(\s*Frame\s*\*\s*current\s*,\s*Frame\s*\*\s*last\s*,\s*const\s+SE3\s*&\s*velocity\s*,\s*PoseOptimizer\s*&\s*opt\s*\)",
                 r"int\s+LocalKeyFrames\s*\(\s*Frame\s*\*\s*current\s*,\s*std::vector<Frame\s*\*>\s*\*\s*out\s*\)",
                 r"int\s+TrackLocalMap\s*\(\s*Frame\s*\*\s*current\s*,\s*const\s+std::vector<Frame\s*\*>\s*&\s*local_keyframes\s*,\s*PoseOptimizer\s*&\s*opt\s*\)",
                 r"void\s+SetURight\s*\(\s*const\s+Frame\s*\*", r"void\s+ClearURight\s*\(", r"void\s+Clear\s*\(\s*\)", r"GetSearch\s*\(\s*int\s+which\s*\)\s*const",
                 r"GetStats\s*\(\s*\)\s*const", r"WITHOUT the spanning tree"]:
        assert re.search(decl, hdr), decl
    opts = [("_baseline", "0.1"), ("_th_motion", "7.0"), ("_th_local", "1.0"), ("_th_dist", "100"), ("_ratio", "0.8"), ("_check_orientation", "true"),
            ("_min_matches_motion", "20"), ("_local_keyframes_max", "80"), ("_neighbours", "10")]
    at = -1
    for opt, val in opts:
        m = re.search(r"\b%s\s*=\s*%s\s*;" % (opt, re.escape(val)), hdr)
        assert m and m.start() > at, opt
        at = m.start()
    assert '#include "ygz/Algorithm/StereoTracker.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_strack.cpp") == 2
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_strack.cpp")).read())
    # one entry point, called from one place; the other classes are used, not changed; _last_seen belongs to the mapper; the point sets of
    # this surface, of ygz_slm.cpp and of ygz_lfuse.cpp go through ONE gather in surface_share.cpp (ygz_proj.cpp defines the function and
    # keeps its own rule for skipped points)
    assert host.count("ygz_hip_stereo_track_search(") == 1 and host.count("PointAttributes(") == 0 and host.count("opt.Optimize(") == 2
    hostdir = os.path.join(PKG, "host")
    calls = {f: re.sub(r"//[^\n]*", "", open(os.path.join(hostdir, f)).read()).count("PointAttributes(")
             for f in os.listdir(hostdir) if f.endswith((".cpp", ".h")) and f != "ygz_proj.cpp"}
    assert calls["surface_share.cpp"] == 1 and sum(calls.values()) == 1, calls
    assert calls["ygz_slm.cpp"] == 0 and calls["ygz_lfuse.cpp"] == 0
    assert "_last_seen" not in host and "ygz_hip_search_by_projection" not in host and "ygz_hip_local_fuse_search" not in host
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code, path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.STRACK_SYMBOLS == ["ygz_hip_default_strack_params", "ygz_hip_stereo_track_search"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: the stereo tracking search added", hdr) and hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for s in hip_lib.STRACK_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    L = st.lib()
    for k, (name, val, py) in enumerate([("MAX_PROBLEMS", 64, hip_lib.STRACK_MAX_PROBLEMS), ("MAX_SETS", 8, hip_lib.STRACK_MAX_SETS),
                                         ("MAX_PAIRS", 262144, hip_lib.STRACK_MAX_PAIRS), ("TOPK", 8, hip_lib.STRACK_TOPK)]):
        assert re.search(r"#define\s+YGZ_STRACK_%s\s+%d\b" % (name, val), hdr) and py == val == getattr(st, name) == L.st_limit(k)
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"SCR_STRACK == 41", internal) and re.search(r"SCR_LFUSE == 40", internal) and "KID_STRACK_SEARCH" in internal
    assert '"k_strack_search"' in open(os.path.join(PKG, "csrc", "ctx.hip")).read()
    for which, (mine, ref, size, fn, names) in enumerate([(hip_lib.StrackPoints, st.Points, 56, L.st_points_size, st.POINTS_FIELDS),
                                                          (hip_lib.StrackProblem, st.Problem, 136, L.st_problem_size, st.PROBLEM_FIELDS),
                                                          (hip_lib.StrackParams, st.Params, 48, L.st_params_size, st.PARAM_FIELDS)]):
        assert [n for n, _ in mine._fields_] == [n for n, _ in ref._fields_] == names
        assert ctypes.sizeof(mine) == ctypes.sizeof(ref) == fn() == size
        for k, (n, _) in enumerate(mine._fields_):
            assert getattr(mine, n).offset == getattr(ref, n).offset == L.st_offset(which, k), n
    assert re.search(r"sizeof: ygz_strack_params 48, ygz_strack_points 56, ygz_strack_problem 136", hdr)


def test_defaults(hip_lib):
    lib = hip_lib.load()
    hip_lib.strack_argtypes(lib)
    p = hip_lib.StrackParams()
    p.check_orientation = 7
    lib.ygz_hip_default_strack_params(ctypes.byref(p))
    lib.ygz_hip_default_strack_params(None)                                          # no effect, no crash
    assert bytes(p) == bytes(st.default_params())
    assert (p.baseline, p.ratio, p.r_near, p.r_wide, p.cos_near, p.th_dist, p.check_orientation) == (0.1, 0.8, 2.5, 4.0, 0.998, 100, 1)


def bad_params():
    out = [dict(th_dist=-1), dict(th_dist=257)]
    for name in ("baseline", "ratio", "r_near", "r_wide"):
        out += [{name: 0.0}, {name: -1.0}, {name: float("nan")}, {name: float("inf")}]
    return out + [dict(cos_near=float("nan"))]


def test_every_invalid_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.strack_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    fs, fp = st.frame_scene(12, 9, 3, skip=True, taken=True)
    ls, lp = st.local_scene(12, 9, 4, skip=True, taken=True)
    s, p, sl, pl = fs[0], fp[0], ls[0], dict(lp[0], set=1)
    K = np.array(st.K4_DEFAULT)
    out = [np.zeros(256, np.int32) for _ in range(7)]
    proj, cand, counts, rot = np.zeros(256), np.zeros(256, np.int32), np.zeros(64 * 4, np.int32), np.zeros(64 * 33, np.int32)

    def call(sets=(s, sl), problems=(p, pl), n_sets=None, n_problems=None, K4=K, params=None, sets_null=False, problems_null=False):
        sa, pa, keep = st.c_arrays(list(sets), list(problems), hip_lib.StrackPoints, hip_lib.StrackProblem)
        f = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None
        return lib.ygz_hip_stereo_track_search(None, len(sets) if n_sets is None else n_sets, None if sets_null else sa,
                                               len(problems) if n_problems is None else n_problems, None if problems_null else pa,
                                               f(K4, ctypes.c_double), ctypes.byref(params) if params is not None else None,
                                               *[f(o, ctypes.c_int32) for o in out], f(proj, ctypes.c_double), f(cand, ctypes.c_int32),
                                               f(counts, ctypes.c_int32), f(rot, ctypes.c_int32))
    assert call() == INV                                                         # valid: only the context is missing
    assert call(params=st.params(hip_lib.StrackParams)) == INV
    assert call(sets_null=True) == INV and call(problems_null=True) == INV and call(K4=None) == INV
    assert call(n_sets=0) == INV and call(n_problems=0) == INV and call(n_sets=-1) == INV and call(n_problems=-1) == INV
    assert call(problems=(p,) * 65) == CAP and call(sets=(s,) * 9) == CAP
    for name in ("pw", "pt_desc"):
        assert call(sets=(dict(s, **{name: None}, force_n=12), sl)) == INV, name
    assert call(sets=(dict(s, pt_level=None), sl)) == INV                        # a mode's required arrays
    for name in ("pt_dmax", "pt_normal"):
        assert call(sets=(s, dict(sl, **{name: None}))) == INV, name
    assert call(sets=(dict(s, force_n=-1), sl)) == INV
    assert call(problems=({k: v for k, v in p.items() if k != "kp_angle"}, pl)) == INV      # the set has pt_angle
    for name in ("kp_px", "kp_level", "kp_desc"):
        assert call(problems=(dict(p, **{name: None}, force_n_kp=9),)) == INV, name
    assert call(problems=(dict(p, set=2),)) == INV and call(problems=(dict(p, set=-1),)) == INV
    assert call(problems=(dict(p, force_n_kp=0),)) == INV and call(problems=(dict(p, force_n_kp=-3),)) == INV
    assert call(problems=(dict(p, mode=2),)) == INV and call(problems=(dict(p, mode=-1),)) == INV
    assert call(problems=(dict(p, direction=2),)) == INV and call(problems=(dict(p, direction=-2),)) == INV
    for th in (0.0, -1.0, float("nan"), float("inf")):
        assert call(problems=(dict(p, th=th),)) == INV, th
    assert call(problems=(dict(p, force_n_kp=(1 << 20) + 1),)) == CAP            # refused on the count alone: no array is read before
    n = st.MAX_PAIRS // 2 + 1
    big = dict(pw=np.ones((n, 3)), pt_desc=np.zeros((n, 32), np.uint8), pt_level=np.zeros(n, np.int32))
    q = {k: v for k, v in p.items() if k != "pt_skip"}
    assert call(sets=(big,), problems=(q, q)) == CAP and call(sets=(big,), problems=(q,)) == INV
    for bad in (np.nan, np.inf, -np.inf):
        for name, which in (("pw", 0), ("pt_angle", 0), ("pt_dmax", 1), ("pt_normal", 1)):
            sets = [s, sl]
            a = np.array(sets[which][name], np.float64)
            a.reshape(-1)[5] = bad
            sets[which] = dict(sets[which], **{name: a})
            assert call(sets=tuple(sets)) == INV, (name, bad)
        for name in ("kp_ur", "kp_angle"):
            a = np.array(p[name], np.float64)
            a[4] = bad
            assert call(problems=(dict(p, **{name: a}),)) == INV, name
        for k in range(7):
            T = np.array(p["T"])
            T[k] = bad
            assert call(problems=(dict(p, T=T),)) == INV
        for k in range(4):
            K4 = K.copy()
            K4[k] = bad
            assert call(K4=K4) == INV
    assert call(K4=np.array([0.0, 1.0, 1.0, 1.0])) == INV and call(K4=np.array([1.0, -1.0, 1.0, 1.0])) == INV
    for bad in bad_params():
        assert call(params=st.params(hip_lib.StrackParams, **bad)) == INV, bad
