"""The local-map fusion surface without a device: tests/cpp/lfuse_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the C ABI symbols are bound by the loader and exported; ygz_lfuse_params, ygz_lfuse_points and ygz_lfuse_problem have the
size and the field offsets of the restatement's structs; the defaults are the stated ones; every invalid call comes back with its code and a
null context (the context is checked last, so a valid call with a null context is refused too); the new sources read no environment variable."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import lfuse_ref as lf

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "lfuse.hip"), os.path.join(PKG, "host", "ygz_lfuse.cpp"), os.path.join(ROOT, "tests", "cpp", "lfuse_surface.cpp"),
               os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoMapper.h"), os.path.join(ROOT, "tests", "lfuse_ref.c")]


def build_program(out_dir):
    """compile tests/cpp/lfuse_surface.cpp into a program in out_dir (also used by tests/test_gpu_lfuse_surface.py)"""
    exe = os.path.join(out_dir, "lfuse_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lfuse_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoMapper.h")).read()
    for decl in [r"int\s+SearchInNeighbors\s*\(\s*Frame\s*\*\s*kf\s*,\s*Matcher\s*&\s*matcher\s*\)", r"int\s+MapPointCulling\s*\(\s*Frame\s*\*\s*kf\s*\)",
                 r"GetFusions\s*\(\s*\)\s*const", r"GetTouched\s*\(\s*\)\s*const", r"GetStats\s*\(\s*\)\s*const", r"GetRecent\s*\(\s*\)\s*const",
                 r"void\s+ClearRecent\s*\(\s*\)", r"The one difference from ORB-SLAM2, which fuses target by target"]:
        assert re.search(decl, hdr), decl
    # the new options stand behind the existing ones, with the stated defaults
    opts = [("_baseline", "0.1"), ("_chi2_mono", "5.991"), ("_chi2_stereo", "7.8"), ("_cos_parallax_max", "0.9998"), ("_th_depth", "3.5"),
            ("_min_close", "100"), ("_neighbours", "10"), ("_second_neighbours", "5"), ("_fuse_th", "3.0"), ("_fuse_chi2_mono", "5.99"),
            ("_fuse_chi2_stereo", "7.8"), ("_cull_min_obs", "3"), ("_cull_found_ratio", "0.25f")]
    at = -1
    for opt, val in opts:
        m = re.search(r"\b%s\s*=\s*%s\s*;" % (opt, re.escape(val)), hdr)
        assert m and m.start() > at, opt
        at = m.start()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_lfuse.cpp") == 2
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_lfuse.cpp")).read())
    # one entry point, called once per direction through one helper; the replacement rule is LoopClosing's; covisibility is the caller's
    assert host.count("ygz_hip_local_fuse_search(") == 1 and host.count("ReplaceMapPoint(") == 1 and host.count("ComputeDistinctiveDescriptors(") == 1
    assert "UpdateCovisibility" not in host and "ygz_hip_covisibility" not in host and "ygz_hip_search_by_projection" not in host
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code, path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.LFUSE_SYMBOLS == ["ygz_hip_default_lfuse_params", "ygz_hip_local_fuse_search"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: local-map fusion search added", hdr) and hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for s in hip_lib.LFUSE_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    for name, val, py in [("PROBLEMS", 64, hip_lib.LFUSE_MAX_PROBLEMS), ("SETS", 8, hip_lib.LFUSE_MAX_SETS), ("PAIRS", 1048576, hip_lib.LFUSE_MAX_PAIRS)]:
        assert re.search(r"#define\s+YGZ_LFUSE_MAX_%s\s+%d\b" % (name, val), hdr) and py == val == getattr(lf, "MAX_" + name)
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"SCR_LFUSE == 40", internal)
    L = lf.lib()
    for which, (mine, ref, size, fn) in enumerate([(hip_lib.LfusePoints, lf.Points, 40, L.lf_points_size), (hip_lib.LfuseProblem, lf.Problem, 112, L.lf_problem_size),
                                                   (hip_lib.LfuseParams, lf.Params, 40, L.lf_params_size)]):
        assert [n for n, _ in mine._fields_] == [n for n, _ in ref._fields_]
        assert ctypes.sizeof(mine) == ctypes.sizeof(ref) == fn() == size
        for k, (n, _) in enumerate(mine._fields_):
            assert getattr(mine, n).offset == getattr(ref, n).offset == L.lf_offset(which, k), n
    assert [n for n, _ in hip_lib.LfuseParams._fields_] == lf.PARAM_FIELDS


def test_defaults(hip_lib):
    lib = hip_lib.load()
    hip_lib.lfuse_argtypes(lib)
    p = hip_lib.LfuseParams()
    p.pad = 7
    lib.ygz_hip_default_lfuse_params(ctypes.byref(p))
    lib.ygz_hip_default_lfuse_params(None)                                           # no effect, no crash
    assert bytes(p) == bytes(lf.default_params())
    assert (p.th, p.baseline, p.chi2_mono, p.chi2_stereo, p.th_dist, p.pad) == (3.0, 0.1, 5.99, 7.8, 50, 0)


def test_every_invalid_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.lfuse_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    sets, pbs = lf.shared_scene(12, 9, 2, 3)
    s, p = sets[0], pbs[0]
    K = np.array(lf.K4_DEFAULT)
    out = [np.zeros(64, np.int32) for _ in range(6)]

    def call(sets=(s,), problems=(p, pbs[1]), n_sets=None, n_problems=None, K4=K, params=None, sets_null=False, problems_null=False):
        sa, pa, keep = lf.c_arrays(list(sets), list(problems), hip_lib.LfusePoints, hip_lib.LfuseProblem)
        f = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None
        return lib.ygz_hip_local_fuse_search(None, len(sets) if n_sets is None else n_sets, None if sets_null else sa,
                                             len(problems) if n_problems is None else n_problems, None if problems_null else pa,
                                             f(K4, ctypes.c_double), ctypes.byref(params) if params is not None else None,
                                             *[f(o, ctypes.c_int32) for o in out])
    assert call() == INV                                                         # valid: only the context is missing
    assert call(params=lf.params(hip_lib.LfuseParams)) == INV
    assert call(sets_null=True) == INV and call(problems_null=True) == INV and call(K4=None) == INV
    assert call(n_sets=0) == INV and call(n_problems=0) == INV and call(n_sets=-1) == INV and call(n_problems=-1) == INV
    assert call(problems=(p,) * 65) == CAP and call(sets=(s,) * 9) == CAP
    for name in ("pw", "pt_desc", "pt_dmax"):
        assert call(sets=(dict(s, **{name: None}, force_n=12),)) == INV, name
    assert call(sets=(dict(s, force_n=-1),)) == INV
    assert call(sets=(dict(s, pt_normal=None),)) == INV                          # optional: valid, the context is missing
    for name in ("kp_px", "kp_level", "kp_desc"):
        assert call(problems=(dict(p, **{name: None}, force_n_kp=9),)) == INV, name
    assert call(problems=(dict(p, set=1),)) == INV and call(problems=(dict(p, set=-1),)) == INV
    assert call(problems=(dict(p, force_n_kp=0),)) == INV and call(problems=(dict(p, force_n_kp=-3),)) == INV
    assert call(problems=(dict(p, force_n_kp=(1 << 20) + 1),)) == CAP            # refused on the count alone: no array is read before
    n = lf.MAX_PAIRS // 2 + 1
    big = dict(pw=np.ones((n, 3)), pt_desc=np.zeros((n, 32), np.uint8), pt_dmax=np.ones(n))
    q = {k: v for k, v in p.items() if k != "pt_skip"}
    assert call(sets=(big,), problems=(q, q)) == CAP and call(sets=(big,), problems=(q,)) == INV
    for bad in (np.nan, np.inf, -np.inf):
        for name in ("pw", "pt_dmax"):
            a = np.array(s[name], np.float64)
            a.reshape(-1)[5] = bad
            assert call(sets=(dict(s, **{name: a}),)) == INV, (name, bad)
        a = np.array(p["kp_ur"])
        a[4] = bad
        assert call(problems=(dict(p, kp_ur=a),)) == INV
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
        assert call(params=lf.params(hip_lib.LfuseParams, **bad)) == INV, bad


def bad_params():
    out = [dict(th_dist=-1), dict(th_dist=257)]
    for name in ("th", "baseline", "chi2_mono", "chi2_stereo"):
        out += [{name: 0.0}, {name: -1.0}, {name: float("nan")}, {name: float("inf")}]
    return out
