"""The local-map selection surface without a device: tests/cpp/lms_surface.cpp, written against include/ygz only, compiles and links with
-Wl,--no-undefined; the class header compiles on its own against include/ygz; the C ABI symbols are bound by the loader, exported and
declared; ygz_lms_params has the same size, field offsets and defaults in the header and in _lib.py, and the limits are the same in the header,
in _lib.py and in tests/lms_ref.py; every invalid call comes back with its code and a null context, in the order the header states (the
context is checked last, so a valid call with a null context is refused too); the block's scratch id is 46, outside the enum; the kernel ids
and names are registered in the same order; the new sources read no environment variable."""
import ctypes
import os
import re
import subprocess

import numpy as np

import lms_ref
from conftest import ROOT
from test_svo_surface_build import struct_from_header

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "lms.hip"), os.path.join(PKG, "csrc", "lms_index.h"), os.path.join(PKG, "host", "ygz_lms.cpp"),
               os.path.join(ROOT, "tests", "cpp", "lms_surface.cpp"), os.path.join(ROOT, "tests", "cpp", "lms_index_host.cpp"),
               os.path.join(ROOT, "include", "ygz", "Algorithm", "LocalMapSelector.h"), os.path.join(ROOT, "tests", "lms_ref.py"),
               os.path.join(ROOT, "tests", "lms_ref.c"), os.path.join(ROOT, "tools", "lms_bench.py")]


def build_program(out_dir):
    """compile tests/cpp/lms_surface.cpp into a program in out_dir (also used by tests/test_gpu_lms_surface.py)"""
    exe = os.path.join(out_dir, "lms_surface")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "lms_surface.cpp"), "-o", exe, "-L", PKG, "-lygz_host", "-lygz_hip",
                           "-Wl,--no-undefined", "-Wl,-rpath," + PKG])
    return exe


def test_program_compiles_and_links(tmp_path):
    assert os.path.exists(os.path.join(PKG, "libygz_host.so")), "libygz_host.so is not built (run __graft_entry__.build())"
    exe = build_program(str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # no arguments: the usage line, no device touched
    assert r.returncode == 2 and "usage" in r.stderr


def test_class_header_compiles_against_include_ygz(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "ygz/Algorithm/LocalMapSelector.h"\n'
                   'int main() { ygz::LocalMapSelector s; ygz::LocalMapSelector::Result r; return s._options._neighbours == 10 && !r.keyframes ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_public_surface():
    hdr = open(os.path.join(ROOT, "include", "ygz", "Algorithm", "LocalMapSelector.h")).read()
    for decl in [r"int\s+Select\s*\(\s*const\s+std::vector<Frame\s*\*>\s*&\s*frames\s*,\s*std::vector<Result>\s*\*\s*results\s*\)", r"struct\s+Result\b",
                 r"const\s+std::vector<Frame\s*\*>\s*\*\s*keyframes", r"const\s+std::vector<MapPoint\s*\*>\s*\*\s*points", r"Frame\s*\*\s*ref\b",
                 r"int\s+voters\b", r"int\s+cut\b", r"struct\s+Stats\b", r"creates\s+and changes no point and no keyframe"]:
        assert re.search(decl, hdr), decl
    at = -1
    for opt, val in [("_neighbours", "10"), ("_local_keyframes_max", "80"), ("_max_points", "16384")]:
        m = re.search(r"\b%s\s*=\s*%s\s*;" % (opt, re.escape(val)), hdr)
        assert m and m.start() > at, opt
        at = m.start()
    assert '#include "ygz/Algorithm/LocalMapSelector.h"' in open(os.path.join(ROOT, "include", "ygz", "Algorithm.h")).read()
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert mk.count("ygz_lms.cpp") == 2
    host = re.sub(r"//[^\n]*", "", open(os.path.join(PKG, "host", "ygz_lms.cpp")).read())
    # one entry point, called from one place; no point and no keyframe is made or edited; no other surface is called
    assert host.count("ygz_hip_local_map_select(") == 1 and '#include "surface_share.h"' in host
    for word in ("Memory::Register", "CreateMapPoint", "_cnt_visible", "_cnt_found", "_track_in_view", "->_bad =", "_mappoint =", "StereoTracker",
                 "StereoLocalMap", "ygz_hip_covisibility", "ygz_hip_stereo_local_map_slots"):
        assert word not in host, word
    others = [f for f in os.listdir(os.path.join(PKG, "host")) if f.endswith(".cpp") and f != "ygz_lms.cpp"]
    assert all("ygz_hip_local_map_select" not in open(os.path.join(PKG, "host", f)).read() for f in others)
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code and "environ" not in code, path


def test_symbols_are_bound_and_exported(hip_lib):
    lib = hip_lib.load()
    assert hip_lib.LMS_SYMBOLS == ["ygz_hip_default_lms_params", "ygz_hip_local_map_select"]
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert re.search(r"Still 6: local-map selection added", hdr)
    assert hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version() and re.search(r"#define\s+YGZ_HIP_ABI_VERSION\s+6\b", hdr)
    for s in hip_lib.LMS_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\b(int|void)\s+%s\s*\(" % s, hdr), s
    for name, value, bound, ref in (("KEYFRAMES", 4096, hip_lib.LMS_MAX_KEYFRAMES, lms_ref.MAX_KEYFRAMES), ("COV", 32, hip_lib.LMS_MAX_COV, lms_ref.MAX_COV),
                                    ("FRAMES", 1024, hip_lib.LMS_MAX_FRAMES, lms_ref.MAX_FRAMES),
                                    ("FEATURES", 32768, hip_lib.LMS_MAX_FEATURES, lms_ref.MAX_FEAT)):
        assert re.search(r"#define\s+YGZ_LMS_MAX_%s\s+%d\b" % (name, value), hdr) and bound == value == ref, name
    assert lms_ref.MAX_FRAME_ENTRIES == hip_lib.LMS_MAX_FEATURES and hip_lib.LMS_OUTPUTS == lms_ref.OUTPUTS
    assert hip_lib.LMS_MAX_KEYFRAMES == hip_lib.MAP_MAX_KEYFRAMES and hip_lib.LMS_MAX_FRAMES == hip_lib.SLM_MAX_FRAMES
    assert re.search(r"#define\s+YGZ_LMS_FEAT_END\s+32768\b", open(os.path.join(PKG, "csrc", "lms_index.h")).read())
    # the scratch enum is as it was; the new block's id stands outside it, behind srl.hip's 45 and inside the context's table
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"#define\s+YGZ_N_SCRATCH\s+48\b", internal) and "SCR_LMS" not in internal and "SCR_SRL" not in internal
    lms = open(os.path.join(PKG, "csrc", "lms.hip")).read()
    assert re.search(r"#define\s+SCR_LMS\s+46\b", lms) and "ygz_blob_open(ctx, SCR_LMS" in lms
    assert re.search(r"#define\s+SCR_SRL\s+45\b", open(os.path.join(PKG, "csrc", "srl.hip")).read())
    for f in os.listdir(os.path.join(PKG, "csrc")):
        if f.endswith(".hip") and f != "lms.hip":
            text = open(os.path.join(PKG, "csrc", f)).read()
            assert "SCR_LMS" not in text and not re.search(r"ygz_blob_open\(ctx, 46\b", text), f
    # the kernel ids and their names, in the same places of their lists
    ctx = open(os.path.join(PKG, "csrc", "ctx.hip")).read()
    assert "KID_SLM_SCATTER, KID_LMS_VOTE, KID_LMS_POINTS, KID_LMS_PLACE, KID_LMS_PRIOR, KID_SVO_GATHER" in internal
    assert '"k_slm_scatter", "k_lms_vote", "k_lms_points", "k_lms_place", "k_lms_prior", "k_svo_gather"' in ctx
    ids = re.search(r"enum \{ KID_BGR2GRAY = 0,(.*?)KID_COUNT \}", internal, re.S).group(0)
    names = re.search(r"k_kernel_names\[KID_COUNT\] = \{(.*?)\};", ctx, re.S).group(1)
    kids, kernels = re.findall(r"KID_\w+", ids)[:-1], re.findall(r'"(k_\w+)"', names)
    assert len(kids) == len(kernels)
    for kid, kernel in (("KID_LMS_VOTE", "k_lms_vote"), ("KID_LMS_POINTS", "k_lms_points"), ("KID_LMS_PLACE", "k_lms_place"),
                        ("KID_LMS_PRIOR", "k_lms_prior"), ("KID_STRACK_SEARCH", "k_strack_search"), ("KID_SRL_PICK", "k_srl_pick")):
        assert kids.index(kid) == kernels.index(kernel), kid
        assert kernel == "k_strack_search" or kernel == "k_srl_pick" or "%s, %s," % (kid, kernel) in lms


def test_struct_layout_defaults_and_limits(hip_lib, tmp_path):
    """the header's struct, compiled, against the ctypes struct: size, every offset, every default"""
    fields = struct_from_header("ygz_lms_params")
    names = ["max_keyframes", "max_points"]
    assert [f for f, _ in fields] == [n for n, _ in hip_lib.LmsParams._fields_] == [n for n, _ in lms_ref.Params._fields_] == names
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ygz_hip.h"', 'int main(void) {',
             '  printf("%zu %d %d %d %d\\n", sizeof(ygz_lms_params), YGZ_LMS_MAX_KEYFRAMES, YGZ_LMS_MAX_COV, YGZ_LMS_MAX_FRAMES, YGZ_LMS_MAX_FEATURES);']
    lines += ['  printf("%%zu\\n", offsetof(ygz_lms_params, %s));' % f for f in names]
    lines += ['  return 0; }']
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(hip_lib.LmsParams) == ctypes.sizeof(lms_ref.Params) == 8
    assert got[1:5] == [hip_lib.LMS_MAX_KEYFRAMES, hip_lib.LMS_MAX_COV, hip_lib.LMS_MAX_FRAMES, hip_lib.LMS_MAX_FEATURES]
    assert got[5:] == [getattr(hip_lib.LmsParams, n).offset for n in names] == [0, 4]
    assert re.search(r"sizeof: ygz_lms_params 8", open(os.path.join(ROOT, "include", "ygz_hip.h")).read())
    lib = hip_lib.load()
    hip_lib.lms_argtypes(lib)
    p = hip_lib.LmsParams(7, 7)
    lib.ygz_hip_default_lms_params(ctypes.byref(p))
    lib.ygz_hip_default_lms_params(None)                                             # no effect, no crash
    assert (p.max_keyframes, p.max_points) == (80, 16384) == (lms_ref.DEFAULTS["max_keyframes"], lms_ref.DEFAULTS["max_points"])


def test_every_invalid_call_is_refused_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.lms_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def params(**kw):
        p = hip_lib.LmsParams()
        lib.ygz_hip_default_lms_params(ctypes.byref(p))
        for k, v in kw.items():
            getattr(p, k)
            setattr(p, k, v)
        return p

    def call(K=2, C=1, kf_bad=(0, 0), cov=(1, 0), off=(0, 2, 3), kf=(0, 1, 1), feat=(0, 0, 1), fr_off=(0, 2), fr_pt=(0, 1), F=None, P=None, p=None, null=()):
        a = dict(kf_bad=np.array(kf_bad, np.uint8), cov=np.array(cov, np.int32), off=np.array(off, np.int32), kf=np.array(kf, np.int32),
                 feat=np.array(feat, np.int32), fr_off=np.array(fr_off, np.int32), fr_pt=np.array(fr_pt, np.int32))
        F = len(fr_off) - 1 if F is None else F
        P = len(off) - 1 if P is None else P
        out = [np.full(16, 5, np.int32) for _ in lms_ref.OUTPUTS]                     # nothing is written before the context is known
        arg = dict((k, bp(v) if k == "kf_bad" else ip(v)) for k, v in a.items())
        outs = [ip(o) for o in out]
        for k in null:
            if k in arg:
                arg[k] = None
            else:
                outs[lms_ref.OUTPUTS.index(k)] = None
        rc = lib.ygz_hip_local_map_select(None, K, arg["kf_bad"], C, arg["cov"], P, arg["off"], arg["kf"], arg["feat"], None, F, arg["fr_off"],
                                          arg["fr_pt"], None if p is None else ctypes.byref(p), *outs)
        assert all((o == 5).all() for o in out)                                       # a refused call writes nothing
        return rc
    # 0: a valid call: only the context is missing
    assert call() == INV and call(p=params()) == INV and call(C=0, null=("cov",)) == INV and call(fr_off=(0, 0), fr_pt=()) == INV
    for k in ("votes", "ref", "n_voters", "n_pt", "n_cut", "local_pt", "fr_prior"):
        assert call(null=(k,)) == INV, k                                               # optional: still only the context
    # 1: nulls and counts
    for k in ("kf_bad", "off", "kf", "feat", "fr_off", "fr_pt", "n_local", "local_kf", "cov"):
        assert call(null=(k,)) == INV, k
    assert call(K=0) == INV and call(K=-1) == INV and call(C=-1) == INV and call(P=0) == INV and call(F=0) == INV and call(F=-1) == INV
    # 2: capacities, before the parameters; the nulls come before the capacities
    big = hip_lib.LMS_MAX_KEYFRAMES + 1
    assert call(K=big, kf_bad=[0] * big, cov=[-1] * big) == CAP and call(K=big, kf_bad=[0] * big, cov=[-1] * big, p=params(max_keyframes=0)) == CAP
    assert call(K=big - 1, kf_bad=[0] * big, cov=[-1] * big) == INV
    assert call(K=big, kf_bad=[0] * big, cov=[-1] * big, null=("local_kf",)) == INV
    assert call(C=hip_lib.LMS_MAX_COV + 1, cov=[-1] * (2 * hip_lib.LMS_MAX_COV + 2)) == CAP and call(C=hip_lib.LMS_MAX_COV, cov=[-1] * (2 * hip_lib.LMS_MAX_COV)) == INV
    big = hip_lib.LMS_MAX_FRAMES + 1
    assert call(fr_off=[0] * (big + 1), fr_pt=()) == CAP and call(fr_off=[0] * big, fr_pt=(), p=params(max_points=4096)) == INV
    # 3: parameters
    for bad in (dict(max_keyframes=0), dict(max_keyframes=-1), dict(max_keyframes=hip_lib.LMS_MAX_KEYFRAMES + 1), dict(max_points=0), dict(max_points=-3)):
        assert call(p=params(**bad)) == INV, bad
    for fine in (dict(max_keyframes=1), dict(max_keyframes=hip_lib.LMS_MAX_KEYFRAMES), dict(max_points=1), dict(max_points=hip_lib.SLM_MAX_PAIRS)):
        assert call(p=params(**fine)) == INV, fine                                     # the context alone is missing
    # 4: the products, before the offsets are read
    assert call(p=params(max_points=hip_lib.SLM_MAX_PAIRS + 1)) == CAP
    assert call(fr_off=[0] * 5, fr_pt=(), p=params(max_points=hip_lib.SLM_MAX_PAIRS // 4 + 1)) == CAP
    assert call(fr_off=[0] * 5, fr_pt=(), off=(1, 2, 3), p=params(max_points=hip_lib.SLM_MAX_PAIRS // 4 + 1)) == CAP
    assert call(fr_off=[0] * 5, fr_pt=(), p=params(max_points=hip_lib.SLM_MAX_PAIRS // 4)) == INV
    assert hip_lib.LMS_MAX_KEYFRAMES * hip_lib.LMS_MAX_FRAMES == hip_lib.COVIS_MAX_CELLS     # the second product is bounded by the limits of (2)
    # 5: offsets
    assert call(off=(1, 2, 3)) == INV and call(off=(0, 3, 2)) == INV and call(fr_off=(1, 2)) == INV and call(fr_off=(0, 2, 1), fr_pt=(0, 1)) == INV
    # 6: the sizes of the lists, before the lists are read
    n = hip_lib.MAP_MAX_OBS_PER_POINT + 1
    assert call(K=n, kf_bad=[0] * n, cov=[-1] * n, off=(0, n), kf=[0] * n, feat=[0] * n) == CAP
    n = hip_lib.LMS_MAX_FEATURES + 1
    assert call(fr_off=(0, n), fr_pt=[7] * n) == CAP and call(fr_off=(0, n - 1), fr_pt=[0] * (n - 1)) == INV
    # 7: indices
    assert call(kf=(0, 2, 1)) == INV and call(kf=(-1, 1, 1)) == INV and call(kf=(1, 1, 1)) == INV and call(kf=(1, 0, 1)) == INV
    assert call(feat=(0, -1, 1)) == INV and call(feat=(0, hip_lib.LMS_MAX_FEATURES, 1)) == INV
    assert call(cov=(2, 0)) == INV and call(cov=(1, -2)) == INV and call(fr_pt=(0, 2)) == INV and call(fr_pt=(-2, 1)) == INV
