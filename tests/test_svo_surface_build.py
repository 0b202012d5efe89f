"""The stereo odometry surface without a device: tests/cpp/svo_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the C ABI symbols are bound by the loader, exported and declared; ygz_svo_params has the same size, field offsets and
defaults in the header and in _lib.py, and the limit is the same; every invalid call comes back with its code and a null context (the context
is checked last, so a valid call with a null context is refused too); SCR_SVO is 42; the new sources read no environment variable;
ygz_svo.cpp calls the entry point from one place."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "svo.hip"), os.path.join(PKG, "csrc", "strack_dev.h"), os.path.join(PKG, "csrc", "popt_dev.h"),
               os.path.join(PKG, "host", "ygz_svo.cpp"), os.path.join(ROOT, "tests", "cpp", "svo_surface.cpp"),
               os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoOdometry.h"), os.path.join(ROOT, "tests", "svo_ref.py"),
               os.path.join(ROOT, "tools", "svo_bench.py")]


def build_program(out_dir):
    """compile tests/cpp/svo_surface.cpp into a program in out_dir (also used by tests/test_gpu_svo_surface.py)"""
    exe = os.path.join(out_dir, "svo_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "svo_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoOdometry.h")).read()
    for decl in [r"int\s+TrackPairs\s*\(\s*const\s+std::vector<std::pair<Frame\s*\*\s*,\s*Frame\s*\*>>\s*&\s*pairs\s*,\s*const\s+std::vector<SE3>\s*\*\s*guesses\s*,"
                 r"\s*std::vector<Result>\s*\*\s*results\s*\)",
                 r"bool\s+Track\s*\(\s*Frame\s*\*\s*current\s*,\s*Frame\s*\*\s*last\s*,\s*const\s+SE3\s*&\s*guess", r"struct\s+Result\b",
                 r"no _mappoint is read or written"]:
        assert re.search(decl, hdr), decl
    opts = [("_baseline", "0.1"), ("_th", "7.0"), ("_th_dist", "100"), ("_check_orientation", "true"), ("_min_matches", "20"), ("_min_tracked", "10")]
    at = -1
    for opt, val in opts:
        m = re.search(r"\b%s\s*=\s*%s\s*;" % (opt, re.escape(val)), hdr)
        assert m and m.start() > at, opt
        at = m.start()
    assert '#include "ygz/Algorithm/StereoOdometry.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_svo.cpp") == 2
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_svo.cpp")).read())
    # one entry point, called from one place; the slots are filled by the shared loader, called from one place; no map is touched
    assert host.count("ygz_hip_stereo_odometry_slots(") == 1 and host.count("load_slots(") == 1
    assert host.count("ygz_hip_describe_given_angle(") == 0 and host.count("ygz_hip_set_keypoint_depths(") == 0
    for word in ("_mappoint", "Memory::", "ygz_hip_stereo_track_search", "ygz_hip_optimize_pose_stereo", "_obs"):
        assert word not in host, word
    others = [f for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".cpp") and f != "ygz_svo.cpp"]
    assert all("ygz_hip_stereo_odometry_slots" not in open(os.path.join(PKG, "host", f)).read() for f in others)
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code and "environ" not in code, path


def test_slot_loading_is_written_once():
    """host/surface_share.cpp alone puts feature lists and depths into slots (ygz_host.cpp keeps its own describe call for the detector); the
    three slot trackers call its loader once each; good(const MapPoint *) is defined once under host/"""
    hostdir = os.path.join(PKG, "host")
    code = {f: re.sub(r"//[^\n]*", "", open(os.path.join(hostdir, f)).read()) for f in os.listdir(hostdir) if f.endswith((".cpp", ".h"))}
    share = code["surface_share.cpp"] + code["surface_share.h"]
    for call in ("ygz_hip_describe_given_angle(", "ygz_hip_set_keypoint_depths("):
        assert share.count(call) == 1 and code["surface_share.cpp"].count(call) == 1, call
        assert {f for f in code if call in code[f]} <= {"surface_share.cpp", "ygz_host.cpp"}, call
    for f in ("ygz_svo.cpp", "ygz_slm.cpp", "ygz_srk.cpp"):
        assert code[f].count("load_slots(") == 1, f
    assert sum(c.count("good(const MapPoint") for c in code.values()) == 1 and code["surface_share.h"].count("good(const MapPoint") == 1
    mk = open(os.path.join(hostdir, "Makefile")).read()
    assert mk.count("surface_share.cpp") == 2 and mk.count("surface_share.h") == 1


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.SVO_SYMBOLS == ["ygz_hip_default_svo_params", "ygz_hip_stereo_odometry_slots"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: stereo odometry on resident slots added", hdr) and hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for s in hip_lib.SVO_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    assert re.search(r"#define\s+YGZ_SVO_MAX_PAIRS\s+1024\b", hdr) and hip_lib.SVO_MAX_PAIRS == 1024
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"SCR_SVO == 42", internal) and re.search(r"SCR_STRACK == 41", internal) and "SCR_LFUSE, SCR_STRACK, SCR_SVO," in internal
    assert re.search(r"SCR_LAST = SCR_SVO", internal) and "KID_SVO_GATHER, KID_SVO_RESOLVE, KID_SVO_SCATTER, KID_LFUSE_SEARCH, KID_STRACK_SEARCH, KID_COUNT" in internal
    ctx = open(os.path.join(PKG, "csrc", "ctx.hip")).read()
    assert '"k_svo_gather", "k_svo_resolve", "k_svo_scatter", "k_lfuse_search", "k_strack_search"' in ctx
    svo = open(os.path.join(PKG, "csrc", "svo.hip")).read()
    assert "ygz_blob_open(ctx, SCR_SVO" in svo


def struct_from_header(name):
    """(field, C type) of a typedef struct in include/ygz_hip.h, in order"""
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"([\w ]+?)\s+([\w, ]+)$", decl)
        for field in m.group(2).split(","):
            out.append((field.strip(), m.group(1).strip()))
    return out


def test_struct_layout_defaults_and_limit(hip_lib, tmp_path):
    """the header's struct, compiled, against the ctypes struct: size, every offset, every default"""
    fields = struct_from_header("ygz_svo_params")
    assert [f for f, _ in fields] == [n for n, _ in hip_lib.SvoParams._fields_] == ["baseline", "th", "th_dist", "check_orientation", "min_matches", "pad", "pose"]
    pose_fields = [f for f, _ in struct_from_header("ygz_pose_opt_params")]
    assert pose_fields == [n for n, _ in hip_lib.PoseOptParams._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ygz_hip.h"', 'int main(void) {',
             '  printf("%zu %d\\n", sizeof(ygz_svo_params), YGZ_SVO_MAX_PAIRS);']
    lines += ['  printf("%%zu\\n", offsetof(ygz_svo_params, %s));' % f for f, _ in fields]
    lines += ['  printf("%%zu\\n", offsetof(ygz_svo_params, pose.%s));' % f for f in pose_fields]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(got[0]) == ctypes.sizeof(hip_lib.SvoParams) == 88 and int(got[1]) == hip_lib.SVO_MAX_PAIRS
    offs = [int(v) for v in got[2:]]
    want = [getattr(hip_lib.SvoParams, n).offset for n, _ in hip_lib.SvoParams._fields_]
    want += [hip_lib.SvoParams.pose.offset + getattr(hip_lib.PoseOptParams, n).offset for n in pose_fields]
    assert offs == want
    assert re.search(r"sizeof: ygz_svo_params 88", open(os.path.join(ROOT, "include", "ygz_hip.h")).read())
    lib = hip_lib.load()
    hip_lib.svo_argtypes(lib)
    hip_lib.popt_argtypes(lib)
    p = hip_lib.SvoParams()
    p.check_orientation, p.pad = 7, 7
    lib.ygz_hip_default_svo_params(ctypes.byref(p))
    lib.ygz_hip_default_svo_params(None)                                             # no effect, no crash
    assert (p.baseline, p.th, p.th_dist, p.check_orientation, p.min_matches, p.pad) == (0.1, 7.0, 100, 1, 20, 0)
    q = hip_lib.PoseOptParams()
    lib.ygz_hip_default_pose_opt_params(ctypes.byref(q))
    q.baseline = 0.1
    assert bytes(p.pose) == bytes(q) and (q.rounds, q.iterations, q.max_trials, q.robust_rounds, q.min_edges, q.min_inliers) == (4, 10, 10, 3, 3, 10)


def test_every_invalid_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.svo_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)

    def params(**fields):
        p = hip_lib.SvoParams()
        lib.ygz_hip_default_svo_params(ctypes.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p, k)
            getattr(tgt, name)
            setattr(tgt, name, v)
        return p

    def call(last=(0, 1), cur=(1, 2), n=None, T=None, direction=None, p=None, last_null=False, cur_null=False, out_null=False):
        la, ca = np.array(last, np.int32), np.array(cur, np.int32)
        n = len(la) if n is None else n
        out = np.zeros((max(len(la), 1), 7))
        Ta = None if T is None else np.ascontiguousarray(T, np.float64)
        da = None if direction is None else np.ascontiguousarray(direction, np.int32)
        return lib.ygz_hip_stereo_odometry_slots(None, n, None if last_null else la.ctypes.data_as(ip), None if cur_null else ca.ctypes.data_as(ip),
                                                 None if Ta is None else Ta.ctypes.data_as(dp), None if da is None else da.ctypes.data_as(ip),
                                                 None if p is None else ctypes.byref(p), None if out_null else out.ctypes.data_as(dp),
                                                 *([None] * 20))
    assert call() == INV                                                         # valid: only the context is missing
    assert call(p=params()) == INV and call(T=np.tile([0, 0, 0, 1.0, 0, 0, 0], (2, 1)), direction=[1, -1]) == INV
    assert call(last_null=True) == INV and call(cur_null=True) == INV and call(out_null=True) == INV
    assert call(n=0) == INV and call(n=-1) == INV
    big = hip_lib.SVO_MAX_PAIRS + 1
    assert call(last=[0] * big, cur=[1] * big) == CAP and call(last=[0] * (big - 1), cur=[1] * (big - 1)) == INV
    assert call(last=[0] * big, cur=[1] * big, p=params(th=-1.0)) == CAP             # the count is checked before the parameters
    for bad in (dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(th=0.0), dict(th=-7.0),
                dict(th=float("nan")), dict(th=float("inf")), dict(th_dist=-1), dict(th_dist=257), dict(min_matches=-1),
                dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=-1.0), dict(pose_chi2_mono=float("nan")), dict(pose_chi2_stereo=float("inf")),
                dict(pose_min_rel_decrease=float("nan")), dict(pose_rounds=0), dict(pose_rounds=9), dict(pose_iterations=0),
                dict(pose_iterations=65), dict(pose_max_trials=0), dict(pose_max_trials=65)):
        assert call(p=params(**bad)) == INV, bad
    for k in range(7):
        for bad in (np.nan, np.inf, -np.inf):
            T = np.tile([0, 0, 0, 1.0, 0, 0, 0], (2, 1))
            T[1, k] = bad
            assert call(T=T) == INV, (k, bad)
    assert call(direction=[0, 2]) == INV and call(direction=[-2, 0]) == INV
    assert call(last=(0, -1)) == INV and call(cur=(1, -2)) == INV and call(last=(0, 2), cur=(1, 2)) == INV


def test_shared_headers_carry_the_two_kernels():
    """StIn / StSetDev / StProbDev and PoptArgs live in the shared headers with the kernels' prototypes; strack.hip and popt.hip define the
    kernels, svo.hip only launches them"""
    sd = open(os.path.join(PKG, "csrc", "strack_dev.h")).read()
    pd = open(os.path.join(PKG, "csrc", "popt_dev.h")).read()
    for word in ("struct StIn", "struct StSetDev", "struct StProbDev", "__global__ void k_strack_search("):
        assert word in sd, word
    assert "struct PoptArgs" in pd and "__global__ void k_pose_opt(PoptArgs A);" in pd and "const int32_t *end;" in pd
    st, po = open(os.path.join(PKG, "csrc", "strack.hip")).read(), open(os.path.join(PKG, "csrc", "popt.hip")).read()
    assert "struct StProbDev" not in st and '#include "strack_dev.h"' in st and "struct PoptArgs" not in po and '#include "popt_dev.h"' in po
    assert "A.end = nullptr" in po                                       # the array call keeps its contiguous ranges
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert "$(wildcard *.h)" in re.search(r"build/%\.o:[^\n]*", mk).group(0)          # every object depends on every header of csrc/, the two above among them
