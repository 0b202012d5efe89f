"""The stereo reference-keyframe surface without a device: tests/cpp/srk_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the C ABI symbols are bound by the loader, exported and declared; ygz_srk_params has the same size, field offsets and
defaults in the header and in _lib.py, and the three limits are the same; every invalid call comes back with its code and a null context, in
the order the header states (the context is checked last, so a valid call with a null context is refused too); SCR_SRK is 44; the kernel names
stand where their enumerators do; the new sources read no environment variable; ygz_srk.cpp calls the entry point from one place."""
import ctypes
import os
import re
import subprocess

import numpy as np

import srk_ref
from conftest import ROOT
from test_svo_surface_build import struct_from_header

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "srk.hip"), os.path.join(PKG, "csrc", "bow_dev.h"), os.path.join(PKG, "host", "ygz_srk.cpp"),
               os.path.join(ROOT, "tests", "cpp", "srk_surface.cpp"), os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoRefTracker.h"),
               os.path.join(ROOT, "tests", "srk_ref.py"), os.path.join(ROOT, "tools", "srk_bench.py")]


def build_program(out_dir):
    """compile tests/cpp/srk_surface.cpp into a program in out_dir (also used by tests/test_gpu_srk_surface.py)"""
    exe = os.path.join(out_dir, "srk_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "srk_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoRefTracker.h")).read()
    for decl in [r"int\s+TrackReferenceKeyFrame\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*frames\s*,\s*const\s+std::vector<Frame\s*\*>\s*&"
                 r"\s*reference_keyframes\s*,\s*std::vector<Result>\s*\*\s*results\s*\)", r"struct\s+Result\b", r"creates no point and no keyframe"]:
        assert re.search(decl, hdr), decl
    opts = [("_baseline", "0.1"), ("_th_low", "50"), ("_knn_ratio", "0.7f"), ("_levelsup", "4"), ("_check_orientation", "true"),
            ("_min_matches", "15"), ("_min_inliers", "10"), ("_min_tracked", "10")]
    at = -1
    for opt, val in opts:
        m = re.search(r"\b%s\s*=\s*%s\s*;" % (opt, re.escape(val)), hdr)
        assert m and m.start() > at, opt
        at = m.start()
    assert '#include "ygz/Algorithm/StereoRefTracker.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    assert "StereoRefTracker" in open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoTracker.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_srk.cpp") == 2
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_srk.cpp")).read())
    # one entry point, called from one place; the slots are filled by the shared loader, called from one place (test_svo_surface_build.py
    # holds the loader itself); no point and no keyframe is made, and the host-array calls are not used
    assert host.count("ygz_hip_stereo_ref_keyframe_slots(") == 1 and host.count("load_slots(") == 1
    assert host.count("ygz_hip_describe_given_angle(") == 0 and host.count("ygz_hip_set_keypoint_depths(") == 0
    for word in ("Memory::", "CreateMapPoint", "RegisterKeyFrame", "ygz_hip_search_by_bow", "ygz_hip_compute_bow", "ygz_hip_optimize_pose_stereo",
                 "Matcher", "PoseOptimizer", "_cnt_found"):
        assert word not in host, word
    others = [f for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".cpp") and f != "ygz_srk.cpp"]
    assert all("ygz_hip_stereo_ref_keyframe_slots" not in open(os.path.join(PKG, "host", f)).read() for f in others)
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code and "environ" not in code, path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.SRK_SYMBOLS == ["ygz_hip_default_srk_params", "ygz_hip_stereo_ref_keyframe_slots"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: stereo reference-keyframe tracking on resident slots added", hdr)
    assert hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version()
    for phrase in ("Still 6: stereo local-map tracking on resident slots added", "Still 6: stereo odometry on resident slots added",
                   "Still 6: the stereo tracking search added"):
        assert phrase in hdr, phrase
    for s in hip_lib.SRK_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    for name, value, bound, ref in (("FRAMES", 1024, hip_lib.SRK_MAX_FRAMES, srk_ref.MAX_FRAMES),
                                    ("KEYFRAMES", 256, hip_lib.SRK_MAX_KEYFRAMES, srk_ref.MAX_KEYFRAMES),
                                    ("SETS", 64, hip_lib.SRK_MAX_SETS, srk_ref.MAX_SETS)):
        assert re.search(r"#define\s+YGZ_SRK_MAX_%s\s+%d\b" % (name, value), hdr) and bound == value == ref, name
    assert hip_lib.SRK_COUNTS == srk_ref.COUNTS
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"static_assert\(SCR_SRK == 44 && SCR_SRK < YGZ_N_SCRATCH", internal) and re.search(r"SCR_LAST = SCR_SVO \+ 1,[^\n]*\n\s*SCR_SRK \}", internal)
    assert re.search(r"SCR_LAST == SCR_SLM", internal) and "SCR_STRACK, SCR_SVO, SCR_SLM," in internal
    assert "KID_SRK_GATHER, KID_SRK_RESOLVE, KID_SRK_SCATTER, KID_SLM_GATHER, KID_SLM_RESOLVE, KID_SLM_SCATTER," in internal
    ctx = open(os.path.join(PKG, "csrc", "ctx.hip")).read()
    assert '"k_srk_gather", "k_srk_resolve", "k_srk_scatter", "k_slm_gather",' in ctx
    # the enumerators and the names are in the same order
    ids = re.search(r"enum \{ KID_BGR2GRAY = 0,(.*?)KID_COUNT \}", internal, re.S).group(0)
    names = re.search(r"k_kernel_names\[KID_COUNT\] = \{(.*?)\};", ctx, re.S).group(1)
    kids, kernels = re.findall(r"KID_\w+", ids)[:-1], re.findall(r'"(k_\w+)"', names)
    assert len(kids) == len(kernels)
    for kid, kernel in (("KID_SRK_GATHER", "k_srk_gather"), ("KID_SRK_RESOLVE", "k_srk_resolve"), ("KID_SRK_SCATTER", "k_srk_scatter"),
                        ("KID_SLM_GATHER", "k_slm_gather"), ("KID_BOW_TRANSFORM", "k_bow_transform"), ("KID_BOW_MATCH", "k_bow_match"),
                        ("KID_POSE_OPT", "k_pose_opt"), ("KID_STRACK_SEARCH", "k_strack_search")):
        assert kids.index(kid) == kernels.index(kernel), kid
    srk = open(os.path.join(PKG, "csrc", "srk.hip")).read()
    assert "ygz_blob_open(ctx, SCR_SRK" in srk


def test_struct_layout_defaults_and_limits(hip_lib, tmp_path):
    """the header's struct, compiled, against the ctypes struct: size, every offset, every default"""
    fields = struct_from_header("ygz_srk_params")
    names = ["baseline", "th_low", "knn_ratio", "levelsup", "check_orientation", "min_matches", "min_inliers", "pose"]
    assert [f for f, _ in fields] == [n for n, _ in hip_lib.SrkParams._fields_] == names
    pose_fields = [f for f, _ in struct_from_header("ygz_pose_opt_params")]
    assert pose_fields == [n for n, _ in hip_lib.PoseOptParams._fields_]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ygz_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d %d\\n", sizeof(ygz_srk_params), YGZ_SRK_MAX_FRAMES, YGZ_SRK_MAX_KEYFRAMES, YGZ_SRK_MAX_SETS);']
    lines += ['  printf("%%zu\\n", offsetof(ygz_srk_params, %s));' % f for f, _ in fields]
    lines += ['  printf("%%zu\\n", offsetof(ygz_srk_params, pose.%s));' % f for f in pose_fields]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(got[0]) == ctypes.sizeof(hip_lib.SrkParams) == 88
    assert [int(v) for v in got[1:4]] == [hip_lib.SRK_MAX_FRAMES, hip_lib.SRK_MAX_KEYFRAMES, hip_lib.SRK_MAX_SETS]
    offs = [int(v) for v in got[4:]]
    want = [getattr(hip_lib.SrkParams, n).offset for n, _ in hip_lib.SrkParams._fields_]
    want += [hip_lib.SrkParams.pose.offset + getattr(hip_lib.PoseOptParams, n).offset for n in pose_fields]
    assert offs == want
    # no implicit padding: the fields' sizes add up to the struct's
    assert sum(ctypes.sizeof(t) for _, t in hip_lib.SrkParams._fields_) == 88
    assert re.search(r"sizeof: ygz_srk_params 88", open(os.path.join(ROOT, "include", "ygz_hip.h")).read())
    lib = hip_lib.load()
    hip_lib.srk_argtypes(lib)
    hip_lib.popt_argtypes(lib)
    p = hip_lib.SrkParams()
    p.th_low, p.min_matches = 7, 7
    lib.ygz_hip_default_srk_params(ctypes.byref(p))
    lib.ygz_hip_default_srk_params(None)                                             # no effect, no crash
    assert (p.baseline, p.th_low, p.knn_ratio, p.levelsup, p.check_orientation, p.min_matches, p.min_inliers) == (0.1, 50, np.float32(0.7), 4, 1, 15, 10)
    assert {k: (float(np.float32(v)) if k == "knn_ratio" else v) for k, v in srk_ref.DEFAULTS.items()} == {k: getattr(p, k) for k in srk_ref.DEFAULTS}
    q = hip_lib.PoseOptParams()
    lib.ygz_hip_default_pose_opt_params(ctypes.byref(q))
    q.baseline = 0.1
    assert bytes(p.pose) == bytes(q) and (q.rounds, q.iterations, q.max_trials, q.robust_rounds, q.min_edges, q.min_inliers) == (4, 10, 10, 3, 3, 10)


def test_every_invalid_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.srk_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    I = [0, 0, 0, 1.0, 0, 0, 0]
    CELLS = 16                                                                     # nothing reads kf_point before the context is known

    def params(**fields):
        p = hip_lib.SrkParams()
        lib.ygz_hip_default_srk_params(ctypes.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p, k)
            getattr(tgt, name)
            setattr(tgt, name, v)
        return p

    def a_set(n=5, drop=False, n_pt=None, nan=False):
        pw = np.ones((n, 3))
        if nan:
            pw[n - 1, 1] = np.nan
        s = hip_lib.StrackPoints()
        s.pw = pw.ctypes.data_as(dp)
        if drop:
            s.pw = dp()
        s.n_pt = n if n_pt is None else n_pt
        return s, pw

    def call(sets=None, n_sets=None, kf_slot=(0,), kf_set=(0,), n_kf=None, slot=(1, 2), kf=(0, 0), n=None, T=None, p=None, null=()):
        made = [a_set()] if sets is None else sets
        sa = (hip_lib.StrackPoints * max(len(made), 1))(*[m[0] for m in made])
        ks, kt = np.array(kf_slot, np.int32), np.array(kf_set, np.int32)
        sl, kk = np.array(slot, np.int32), np.array(kf, np.int32)
        n = len(sl) if n is None else n
        n_kf = len(ks) if n_kf is None else n_kf
        kp = np.full((max(len(ks), 1), CELLS), -1, np.int32)
        Ta = np.ascontiguousarray(np.tile(I, (max(len(sl), 1), 1)) if T is None else T, np.float64)
        out = np.zeros((max(len(sl), 1), 7))
        arg = dict(sets=sa, kf_slot=ks.ctypes.data_as(ip), kf_set=kt.ctypes.data_as(ip), kf_point=kp.ctypes.data_as(ip), slot=sl.ctypes.data_as(ip),
                   kf=kk.ctypes.data_as(ip), T=Ta.ctypes.data_as(dp), out=out.ctypes.data_as(dp))
        for k in null:
            arg[k] = None
        return lib.ygz_hip_stereo_ref_keyframe_slots(None, len(made) if n_sets is None else n_sets, arg["sets"], n_kf, arg["kf_slot"], arg["kf_set"],
                                                     arg["kf_point"], n, arg["slot"], arg["kf"], arg["T"], None if p is None else ctypes.byref(p),
                                                     arg["out"], *([None] * 16))
    # 0: a valid call: only the context is missing
    assert call() == INV and call(p=params()) == INV and call(sets=[a_set(0, n_pt=0)]) == INV      # a set of 0 points is a valid set
    # 1: nulls and counts
    for k in ("sets", "kf_slot", "kf_set", "kf_point", "slot", "kf", "T", "out"):
        assert call(null=(k,)) == INV, k
    assert call(n=0) == INV and call(n=-1) == INV and call(n_sets=0) == INV and call(n_sets=-1) == INV and call(n_kf=0) == INV and call(n_kf=-1) == INV
    # 2: capacities, before the parameters
    big = hip_lib.SRK_MAX_FRAMES + 1
    assert call(slot=[1] * big, kf=[0] * big) == CAP and call(slot=[1] * (big - 1), kf=[0] * (big - 1)) == INV
    assert call(slot=[1] * big, kf=[0] * big, p=params(baseline=-1.0)) == CAP
    big = hip_lib.SRK_MAX_KEYFRAMES + 1
    assert call(kf_slot=[0] * big, kf_set=[0] * big) == CAP and call(kf_slot=[0] * (big - 1), kf_set=[0] * (big - 1)) == INV
    one = a_set()
    assert call(sets=[one] * (hip_lib.SRK_MAX_SETS + 1)) == CAP and call(sets=[one] * hip_lib.SRK_MAX_SETS) == INV
    assert call(sets=[one] * (hip_lib.SRK_MAX_SETS + 1), null=("T",)) == INV                 # the nulls come before the capacities
    # 3: parameters
    for bad in (dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(th_low=-1), dict(th_low=257),
                dict(knn_ratio=0.0), dict(knn_ratio=-0.5), dict(knn_ratio=float("nan")), dict(knn_ratio=float("inf")), dict(levelsup=-1),
                dict(min_matches=-1), dict(min_inliers=-1), dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=-1.0), dict(pose_chi2_mono=float("nan")),
                dict(pose_chi2_stereo=float("inf")), dict(pose_min_rel_decrease=float("nan")), dict(pose_rounds=0), dict(pose_rounds=9),
                dict(pose_iterations=0), dict(pose_iterations=65), dict(pose_max_trials=0), dict(pose_max_trials=65)):
        assert call(p=params(**bad)) == INV, bad
    for fine in (dict(th_low=0), dict(th_low=256), dict(levelsup=0), dict(min_matches=0), dict(min_inliers=0), dict(check_orientation=0)):
        assert call(p=params(**fine)) == INV, fine                                           # the context alone is missing
    # 4: sets, slots, indices
    assert call(sets=[a_set(n_pt=-1)]) == INV and call(sets=[a_set(drop=True)]) == INV
    assert call(slot=(1, -1)) == INV and call(kf_slot=(-1,)) == INV and call(kf_set=(1,)) == INV and call(kf_set=(-1,)) == INV
    assert call(kf=(0, 1)) == INV and call(kf=(-1, 0)) == INV
    # 5: a non-finite T or pw
    for k in range(7):
        for bad in (np.nan, np.inf, -np.inf):
            T = np.tile(I, (2, 1))
            T[1, k] = bad
            assert call(T=T) == INV, (k, bad)
    assert call(sets=[a_set(nan=True)]) == INV
