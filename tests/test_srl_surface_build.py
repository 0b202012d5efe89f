"""The stereo relocalisation surface without a device: tests/cpp/srl_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the C ABI symbols are bound by the loader, exported and declared; ygz_srl_params has the same size, field offsets and
defaults in the header and in _lib.py, and the limits are the same; every invalid call comes back with its code and a null context, in the
order the header states (the context is checked last, so a valid call with a null context is refused too); the block's scratch id is 45,
outside the enum that ends in SCR_SRK; the new sources read no environment variable; ygz_srl.cpp calls the entry point from one place and
shares the retrieval with ygz_reloc.cpp."""
import ctypes
import os
import re
import subprocess

import numpy as np

import srl_ref
from conftest import ROOT
from test_svo_surface_build import struct_from_header

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "srl.hip"), os.path.join(PKG, "csrc", "pnp_dev.h"), os.path.join(PKG, "csrc", "cvrng_dev.h"),
               os.path.join(PKG, "host", "ygz_srl.cpp"), os.path.join(PKG, "host", "retrieval.cpp"), os.path.join(PKG, "host", "retrieval.h"),
               os.path.join(ROOT, "tests", "cpp", "srl_surface.cpp"), os.path.join(ROOT, "tests", "cpp", "cvrng_host.cpp"),
               os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoRelocalizer.h"), os.path.join(ROOT, "tests", "srl_ref.py"),
               os.path.join(ROOT, "tools", "srl_bench.py")]


def build_program(out_dir):
    """compile tests/cpp/srl_surface.cpp into a program in out_dir (also used by tests/test_gpu_srl_surface.py)"""
    exe = os.path.join(out_dir, "srl_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "srl_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "StereoRelocalizer.h")).read()
    for decl in [r"int\s+Relocalize\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*frames\s*,\s*const\s+std::vector<std::vector<Frame\s*\*>>\s*&"
                 r"\s*candidates\s*,\s*std::vector<Result>\s*\*\s*results\s*\)",
                 r"std::vector<Frame\s*\*>\s+Candidates\s*\(\s*Frame\s*\*\s*frame\s*,\s*const\s+std::vector<Frame\s*\*>\s*&\s*keyframes\s*\)",
                 r"struct\s+Result\b", r"void\s+SetKeyFrameDatabase\s*\(", r"creates no point and no keyframe"]:
        assert re.search(decl, hdr), decl
    opts = [("_baseline", "0.1"), ("_th_low", "50"), ("_knn_ratio", "0.75f"), ("_levelsup", "4"), ("_check_orientation", "true"),
            ("_min_matches", "15"), ("_ransac_iterations", "300"), ("_ransac_chi2", "5.991"), ("_min_ransac_inliers", "10"),
            ("_min_final_inliers", "50"), ("_max_candidates", "5"), ("_min_score_ratio", "0.75")]
    at = -1
    for opt, val in opts:
        m = re.search(r"\b%s\s*=\s*%s\s*;" % (opt, re.escape(val)), hdr)
        assert m and m.start() > at, opt
        at = m.start()
    assert '#include "ygz/Algorithm/StereoRelocalizer.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_srl.cpp") == 2 and mk.count("retrieval.cpp") == 2 and mk.count("retrieval.h") == 1
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_srl.cpp")).read())
    # one entry point, called from one place; the slots are filled by the shared loader, called from one place; no point and no keyframe is
    # made, and the host-array calls are not used
    assert host.count("ygz_hip_stereo_relocalize_slots(") == 1 and host.count("load_slots(") == 1
    assert host.count("ygz_hip_describe_given_angle(") == 0 and host.count("ygz_hip_set_keypoint_depths(") == 0
    for word in ("Memory::", "CreateMapPoint", "RegisterKeyFrame", "ygz_hip_search_by_bow", "ygz_hip_compute_bow", "ygz_hip_optimize_pose_stereo",
                 "ygz_hip_pnp_ransac", "Matcher", "PoseOptimizer", "_cnt_found"):
        assert word not in host, word
    others = [f for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".cpp") and f != "ygz_srl.cpp"]
    assert all("ygz_hip_stereo_relocalize_slots" not in open(os.path.join(PKG, "host", f)).read() for f in others)
    # the retrieval rule stands once, for both relocalisers
    reloc = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_reloc.cpp")).read())
    assert host.count("hip::bow_candidates(") == 1 and reloc.count("hip::bow_candidates(") == 1
    assert "_vocab->score(" not in reloc and "_vocab->score(" not in host
    assert re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "retrieval.cpp")).read()).count("_vocab->score(") == 1
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code and "environ" not in code, path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.SRL_SYMBOLS == ["ygz_hip_default_srl_params", "ygz_hip_stereo_relocalize_slots"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: stereo relocalisation on resident slots added", hdr)
    assert hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version() and re.search(r"#define\s+YGZ_HIP_ABI_VERSION\s+6\b", hdr)
    for s in hip_lib.SRL_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    for name, value, bound, ref in (("FRAMES", 256, hip_lib.SRL_MAX_FRAMES, srl_ref.MAX_FRAMES),
                                    ("PROBLEMS", 256, hip_lib.SRL_MAX_PROBLEMS, srl_ref.MAX_PROBLEMS),
                                    ("KEYFRAMES", 256, hip_lib.SRL_MAX_KEYFRAMES, srl_ref.MAX_KEYFRAMES),
                                    ("SETS", 64, hip_lib.SRL_MAX_SETS, srl_ref.MAX_SETS),
                                    ("HYPOTHESIS_SETS", 76800, hip_lib.SRL_MAX_HYPOTHESIS_SETS, srl_ref.MAX_HYPOTHESIS_SETS)):
        assert re.search(r"#define\s+YGZ_SRL_MAX_%s\s+%d\b" % (name, value), hdr) and bound == value == ref, name
    assert 76800 * 384 < 32 << 20                                                    # the hypothesis scratch stays at a few tens of MB
    assert hip_lib.SRL_COUNTS == srl_ref.COUNTS and len(hip_lib.SRL_COUNTS) == 10
    assert (hip_lib.SRL_RELOCALISED, hip_lib.SRL_TOO_FEW_MATCHES, hip_lib.SRL_PNP_FAILED, hip_lib.SRL_TOO_FEW_INLIERS) == (
        srl_ref.RELOCALISED, srl_ref.TOO_FEW_MATCHES, srl_ref.PNP_FAILED, srl_ref.TOO_FEW_INLIERS) == (0, 1, 2, 3)
    # the scratch enum is as it was; the new block's id stands outside it, behind SCR_SRK and inside the context's table
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"static_assert\(SCR_SRK == 44 && SCR_SRK < YGZ_N_SCRATCH", internal) and re.search(r"SCR_LAST = SCR_SVO \+ 1,[^\n]*\n\s*SCR_SRK \}", internal)
    assert re.search(r"#define\s+YGZ_N_SCRATCH\s+48\b", internal) and "SCR_SRL" not in internal
    srl = open(os.path.join(PKG, "csrc", "srl.hip")).read()
    assert re.search(r"#define\s+SCR_SRL\s+45\b", srl) and "ygz_blob_open(ctx, SCR_SRL" in srl
    ids = set()
    for f in os.listdir(os.path.join(PKG, "csrc")):
        if f.endswith(".hip") and f != "srl.hip":
            assert "SCR_SRL" not in open(os.path.join(PKG, "csrc", f)).read(), f
            ids |= set(re.findall(r"ygz_blob_open\(ctx, (\w+)", open(os.path.join(PKG, "csrc", f)).read()))
    assert "SCR_SRK" in ids and "45" not in ids
    # the kernel ids and names that the other surfaces pin are as they were
    assert "KID_SRK_GATHER, KID_SRK_RESOLVE, KID_SRK_SCATTER, KID_SLM_GATHER, KID_SLM_RESOLVE, KID_SLM_SCATTER," in internal
    assert '"k_srk_gather", "k_srk_resolve", "k_srk_scatter", "k_slm_gather",' in open(os.path.join(PKG, "csrc", "ctx.hip")).read()


def test_struct_layout_defaults_and_limits(hip_lib, tmp_path):
    """the header's struct, compiled, against the ctypes struct: size, every offset, every default"""
    fields = struct_from_header("ygz_srl_params")
    names = ["baseline", "th_low", "knn_ratio", "levelsup", "check_orientation", "min_matches", "pad0", "pnp", "min_final_inliers", "pad1", "pose"]
    assert [f for f, _ in fields] == [n for n, _ in hip_lib.SrlParams._fields_] == names
    pose_fields = [n for n, _ in hip_lib.PoseOptParams._fields_]
    pnp_fields = [n for n, _ in hip_lib.PnpParams._fields_]
    assert pnp_fields == ["max_iter", "chi2", "min_inliers"]
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ygz_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d %d %d %d\\n", sizeof(ygz_srl_params), YGZ_SRL_MAX_FRAMES, YGZ_SRL_MAX_PROBLEMS, YGZ_SRL_MAX_KEYFRAMES, '
             'YGZ_SRL_MAX_SETS, YGZ_SRL_MAX_HYPOTHESIS_SETS);']
    lines += ['  printf("%%zu\\n", offsetof(ygz_srl_params, %s));' % f for f, _ in fields]
    lines += ['  printf("%%zu\\n", offsetof(ygz_srl_params, pnp.%s));' % f for f in pnp_fields]
    lines += ['  printf("%%zu\\n", offsetof(ygz_srl_params, pose.%s));' % f for f in pose_fields]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert int(got[0]) == ctypes.sizeof(hip_lib.SrlParams) == 120
    assert [int(v) for v in got[1:6]] == [hip_lib.SRL_MAX_FRAMES, hip_lib.SRL_MAX_PROBLEMS, hip_lib.SRL_MAX_KEYFRAMES, hip_lib.SRL_MAX_SETS,
                                          hip_lib.SRL_MAX_HYPOTHESIS_SETS]
    offs = [int(v) for v in got[6:]]
    want = [getattr(hip_lib.SrlParams, n).offset for n, _ in hip_lib.SrlParams._fields_]
    want += [hip_lib.SrlParams.pnp.offset + getattr(hip_lib.PnpParams, n).offset for n in pnp_fields]
    want += [hip_lib.SrlParams.pose.offset + getattr(hip_lib.PoseOptParams, n).offset for n in pose_fields]
    assert offs == want
    # no implicit padding between the fields: their sizes add up to the struct's
    assert sum(ctypes.sizeof(t) for _, t in hip_lib.SrlParams._fields_) == 120
    assert re.search(r"sizeof: ygz_srl_params 120", open(os.path.join(ROOT, "include", "ygz_hip.h")).read())
    lib = hip_lib.load()
    hip_lib.srl_argtypes(lib)
    hip_lib.popt_argtypes(lib)
    p = hip_lib.SrlParams()
    p.th_low, p.min_matches, p.pad0, p.pad1 = 7, 7, 7, 7
    lib.ygz_hip_default_srl_params(ctypes.byref(p))
    lib.ygz_hip_default_srl_params(None)                                             # no effect, no crash
    assert (p.baseline, p.th_low, p.knn_ratio, p.levelsup, p.check_orientation, p.min_matches, p.min_final_inliers, p.pad0, p.pad1) == (
        0.1, 50, np.float32(0.75), 4, 1, 15, 50, 0, 0)
    assert (p.pnp.max_iter, p.pnp.chi2, p.pnp.min_inliers) == (300, 5.991, 10)
    assert srl_ref.DEFAULTS == {k: getattr(p, k) for k in srl_ref.DEFAULTS} and srl_ref.PNP_DEFAULTS == {k: getattr(p.pnp, k) for k in srl_ref.PNP_DEFAULTS}
    q = hip_lib.PoseOptParams()
    lib.ygz_hip_default_pose_opt_params(ctypes.byref(q))
    q.baseline = 0.1
    assert bytes(p.pose) == bytes(q)


def test_every_invalid_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.srl_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    CELLS = 16                                                                     # nothing reads kf_point before the context is known

    def params(**fields):
        p = hip_lib.SrlParams()
        lib.ygz_hip_default_srl_params(ctypes.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p.pnp, k[4:]) if k.startswith("pnp_") else (p, k)
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

    def call(sets=None, n_sets=None, kf_slot=(0,), kf_set=(0,), n_kf=None, slot=(1, 2), off=(0, 1, 3), ckf=(0, 0, 0), n=None, p=None, null=()):
        made = [a_set()] if sets is None else sets
        sa = (hip_lib.StrackPoints * max(len(made), 1))(*[m[0] for m in made])
        ks, kt = np.array(kf_slot, np.int32), np.array(kf_set, np.int32)
        sl, co, ck = np.array(slot, np.int32), np.array(off, np.int32), np.array(ckf, np.int32)
        n = len(sl) if n is None else n
        n_kf = len(ks) if n_kf is None else n_kf
        kp = np.full((max(len(ks), 1), CELLS), -1, np.int32)
        out, best = np.full((max(len(sl), 1), 7), 5.0), np.full(max(len(sl), 1), 5, np.int32)
        arg = dict(sets=sa, kf_slot=ks.ctypes.data_as(ip), kf_set=kt.ctypes.data_as(ip), kf_point=kp.ctypes.data_as(ip), slot=sl.ctypes.data_as(ip),
                   cand_off=co.ctypes.data_as(ip), cand_kf=ck.ctypes.data_as(ip), out=out.ctypes.data_as(dp), best=best.ctypes.data_as(ip))
        for k in null:
            arg[k] = None
        rc = lib.ygz_hip_stereo_relocalize_slots(None, len(made) if n_sets is None else n_sets, arg["sets"], n_kf, arg["kf_slot"], arg["kf_set"],
                                                 arg["kf_point"], n, arg["slot"], arg["cand_off"], arg["cand_kf"],
                                                 None if p is None else ctypes.byref(p), arg["out"], arg["best"], *([None] * 21))
        assert (out == 5.0).all() and (best == 5).all()                             # a refused call writes nothing
        return rc
    # 0: a valid call: only the context is missing
    assert call() == INV and call(p=params()) == INV and call(sets=[a_set(0, n_pt=0)]) == INV      # a set of 0 points is a valid set
    assert call(off=(0, 0, 1), ckf=(0,)) == INV                                     # a frame without candidates is a valid frame
    # 1: nulls and counts
    for k in ("sets", "kf_slot", "kf_set", "kf_point", "slot", "cand_off", "cand_kf", "out", "best"):
        assert call(null=(k,)) == INV, k
    assert call(n=0) == INV and call(n=-1) == INV and call(n_sets=0) == INV and call(n_sets=-1) == INV and call(n_kf=0) == INV and call(n_kf=-1) == INV
    # 2: capacities, before the candidate lists and the parameters
    one = a_set()
    assert call(sets=[one] * (hip_lib.SRL_MAX_SETS + 1)) == CAP and call(sets=[one] * hip_lib.SRL_MAX_SETS) == INV
    assert call(sets=[one] * (hip_lib.SRL_MAX_SETS + 1), null=("best",)) == INV               # the nulls come before the capacities
    big = hip_lib.SRL_MAX_KEYFRAMES + 1
    assert call(kf_slot=[0] * big, kf_set=[0] * big) == CAP and call(kf_slot=[0] * (big - 1), kf_set=[0] * (big - 1)) == INV
    big = hip_lib.SRL_MAX_FRAMES + 1
    assert call(slot=[1] * big, off=list(range(big + 1)), ckf=[0] * big) == CAP
    assert call(slot=[1] * big, off=[5] * (big + 1), ckf=[0] * big, p=params(baseline=-1.0)) == CAP
    # 3: the candidate lists
    assert call(off=(1, 1, 3)) == INV and call(off=(0, 2, 1)) == INV and call(off=(0, 0, 0)) == INV and call(off=(0, -1, 3)) == INV
    big = hip_lib.SRL_MAX_PROBLEMS + 1
    assert call(off=(0, 1, big), ckf=[0] * big) == CAP and call(off=(0, 1, big - 1), ckf=[0] * (big - 1)) == INV
    assert call(off=(0, 1, big), ckf=[0] * big, p=params(th_low=-1)) == CAP
    # 4: parameters
    for bad in (dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(th_low=-1), dict(th_low=257),
                dict(knn_ratio=0.0), dict(knn_ratio=-0.5), dict(knn_ratio=float("nan")), dict(knn_ratio=float("inf")), dict(levelsup=-1),
                dict(min_matches=3), dict(min_matches=-1), dict(min_final_inliers=-1), dict(pnp_max_iter=0), dict(pnp_max_iter=1025),
                dict(pnp_chi2=0.0), dict(pnp_chi2=-1.0), dict(pnp_chi2=float("nan")), dict(pnp_chi2=float("inf")), dict(pnp_min_inliers=-1),
                dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=-1.0), dict(pose_chi2_mono=float("nan")), dict(pose_chi2_stereo=float("inf")),
                dict(pose_min_rel_decrease=float("nan")), dict(pose_rounds=0), dict(pose_rounds=9), dict(pose_iterations=0),
                dict(pose_iterations=65), dict(pose_max_trials=0), dict(pose_max_trials=65)):
        assert call(p=params(**bad)) == INV, bad
    for fine in (dict(th_low=0), dict(th_low=256), dict(levelsup=0), dict(min_matches=4), dict(min_final_inliers=0), dict(check_orientation=0),
                 dict(pnp_max_iter=1), dict(pnp_max_iter=1024), dict(pnp_min_inliers=0)):
        assert call(p=params(**fine)) == INV, fine                                           # the context alone is missing
    # 5: the hypothesis scratch: P * max_iter
    assert call(off=(0, 1, 76), ckf=[0] * 76, p=params(pnp_max_iter=1024)) == CAP and call(off=(0, 1, 75), ckf=[0] * 75, p=params(pnp_max_iter=1024)) == INV
    assert call(off=(0, 1, 256), ckf=[0] * 256) == INV and call(off=(0, 1, 256), ckf=[0] * 256, p=params(pnp_max_iter=301)) == CAP
    assert call(off=(0, 1, 76), ckf=[-1] * 76, p=params(pnp_max_iter=1024)) == CAP              # before the indices
    # 6: sets, slots, indices
    assert call(sets=[a_set(n_pt=-1)]) == INV and call(sets=[a_set(drop=True)]) == INV
    assert call(slot=(1, -1)) == INV and call(kf_slot=(-1,)) == INV and call(kf_set=(1,)) == INV and call(kf_set=(-1,)) == INV
    assert call(ckf=(0, 1, 0)) == INV and call(ckf=(0, 0, -1)) == INV
    # 7: a non-finite pw
    assert call(sets=[a_set(nan=True)]) == INV
