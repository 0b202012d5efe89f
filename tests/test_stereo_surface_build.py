"""The stereo surface without a device: tests/cpp/stereo_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; StereoMatcher is declared and listed in Algorithm.h; the C ABI symbols are bound by the loader and exported; every invalid
call comes back YGZ_E_INVALID with a null context (the context is checked last, so a valid call with a null context is refused too);
ygz_stereo_params has the size and the fields of the restatement's struct and the status codes agree; the new sources read no environment
variable."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import stereo_ref as sr

PKG = os.path.join(ROOT, "ygz_slam_amd")


def build_program(out_dir):
    """compile tests/cpp/stereo_surface.cpp into a program in out_dir (also used by tests/test_gpu_stereo_surface.py)"""
    exe = os.path.join(out_dir, "stereo_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stereo_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoMatcher.h")).read()
    for decl in [r"class\s+StereoMatcher", r"double\s+_baseline\s*=\s*0\.1;", r"double\s+_min_disparity\s*=\s*0;", r"double\s+_max_disparity\s*=\s*0;",
                 r"int\s+_th_dist\s*=\s*75;", r"\}\s*_options;",
                 r"int\s+ComputeStereoMatches\s*\(\s*Frame\s*\*\s*left\s*,\s*Frame\s*\*\s*right\s*,\s*std::vector<double>\s*\*\s*u_right\s*=\s*nullptr\s*\)"]:
        assert re.search(decl, hdr), decl
    assert '#include "ygz/Algorithm/StereoMatcher.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_stereo.cpp") == 2
    host = open(os.path.join(PKG, "host", "ygz_stereo.cpp")).read()
    assert host.count("ygz_hip_stereo_match(") == 1 and "write_depths = 0" in host
    for path in (os.path.join(PKG, "host", "ygz_stereo.cpp"), os.path.join(PKG, "csrc", "stereo.hip"), os.path.join(ROOT, "tests", "cpp", "stereo_surface.cpp")):
        assert "getenv" not in open(path).read(), path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.STEREO_SYMBOLS == ["ygz_hip_default_stereo_params", "ygz_hip_stereo_depths_slots", "ygz_hip_stereo_match", "ygz_hip_stereo_candidates"]
    for s in hip_lib.STEREO_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: stereo input added", hdr) and hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for s in hip_lib.STEREO_SYMBOLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    body = re.search(r"typedef struct \{([^}]*)\} ygz_stereo_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*(double|int)\s+", "", decl.strip()).split(",")]
    assert names == [n for n, _ in hip_lib.StereoParams._fields_] == [n for n, _ in sr.Params._fields_]
    assert ctypes.sizeof(hip_lib.StereoParams) == ctypes.sizeof(sr.Params) == sr.lib().sr_params_size() == 32
    for (n, t), (rn, rtype) in zip(hip_lib.StereoParams._fields_, sr.Params._fields_):
        assert getattr(hip_lib.StereoParams, n).offset == getattr(sr.Params, rn).offset and ctypes.sizeof(t) == ctypes.sizeof(rtype), n
    # the status codes: the header, the loader, the restatement's loader
    codes = ["OK", "NO_CANDIDATE", "DESCRIPTOR", "BORDER", "EDGE", "DISPARITY", "MEDIAN"]
    for v, name in enumerate(codes):
        assert re.search(r"#define\s+YGZ_STEREO_%s\s+%d\b" % (name, v), hdr), name
        assert getattr(hip_lib, "STEREO_" + name) == getattr(sr, name) == v
    assert re.search(r"#define\s+YGZ_STEREO_N_STATUS\s+7\b", hdr) and hip_lib.STEREO_N_STATUS == sr.N_STATUS == 7
    ref = open(os.path.join(ROOT, "tests", "stereo_ref.c")).read()
    assert re.search(r"enum \{ SR_OK = 0, SR_NO_CANDIDATE, SR_DESCRIPTOR, SR_BORDER, SR_EDGE, SR_DISPARITY, SR_MEDIAN, SR_N_STATUS \}", ref)
    # the defaults
    hip_lib.stereo_argtypes(lib)
    p = hip_lib.StereoParams(9.0, 9.0, 9.0, 9, 9)
    lib.ygz_hip_default_stereo_params(ctypes.byref(p))
    assert (p.baseline, p.min_disparity, p.max_disparity, p.th_dist, p.write_depths) == (0.1, 0.0, 0.0, 75, 1) == tuple(sr.fields(sr.params()).values())
    lib.ygz_hip_default_stereo_params(None)


def test_every_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.stereo_argtypes(lib)
    INV = hip_lib.E_INVALID
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    one, two = np.array([0], np.int32), np.array([1], np.int32)
    px, lv, ds = np.zeros((2, 2)), np.zeros(2, np.int32), np.zeros((2, 32), np.uint8)
    kp = (dp(px), ip(lv), bp(ds), 2)

    def prm(**kw):
        v = dict(baseline=0.1, min_disparity=0.0, max_disparity=0.0, th_dist=75, write_depths=1)
        v.update(kw)
        return hip_lib.StereoParams(*[v[n] for n, _ in hip_lib.StereoParams._fields_])

    def calls(p):
        return (lib.ygz_hip_stereo_depths_slots(None, 1, ip(one), ip(two), p, *(None,) * 6),
                lib.ygz_hip_stereo_match(None, 0, 1, *kp, *kp, p, *(None,) * 6),
                lib.ygz_hip_stereo_candidates(None, 0, 1, *kp, *kp, p, *(None,) * 4))
    assert calls(ctypes.byref(prm())) == (INV, INV, INV)                            # valid: only the context is missing
    assert calls(None) == (INV, INV, INV)
    for bad in (dict(baseline=0.0), dict(baseline=-1.0), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(min_disparity=-0.5),
                dict(min_disparity=float("nan")), dict(max_disparity=-2.0), dict(max_disparity=float("inf")), dict(th_dist=-1), dict(th_dist=257)):
        assert calls(ctypes.byref(prm(**bad))) == (INV, INV, INV), bad
