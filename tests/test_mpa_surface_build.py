"""ygz_hip_map_point_attributes and ygz_hip_stereo_local_map_indexed without a device: the symbols are bound by the loader, exported and
declared; the limits are the same in the header, in _lib.py and in tests/mpa_ref.py; every invalid call comes back with its code and a null
context, in the order the header states (the context is checked last, so a valid call with a null context is refused too), and a refused call
writes nothing; the block's scratch id is 47, outside the enum; the new sources read no environment variable."""
import ctypes
import os
import re

import numpy as np

import mpa_ref
from conftest import ROOT

PKG = os.path.join(ROOT, "ygz_slam_amd")
NEW_SOURCES = [os.path.join(PKG, "csrc", "mpa.hip"), os.path.join(PKG, "csrc", "slm_index.hip"), os.path.join(PKG, "csrc", "slm_share.h"),
               os.path.join(ROOT, "tests", "mpa_ref.c"), os.path.join(ROOT, "tests", "mpa_ref.py"), os.path.join(ROOT, "tools", "lmt_bench.py")]
ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
bp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def test_symbols_limits_and_ids(hip_lib):
    lib = hip_lib.load()
    hdr = open(os.path.join(ROOT, "include", "ygz_hip.h")).read()
    assert hip_lib.MPA_SYMBOLS == ["ygz_hip_map_point_attributes", "ygz_hip_stereo_local_map_indexed"]
    assert re.search(r"Still 6: map-point attributes and local-map tracking on an indexed map added", hdr)
    assert hip_lib.ABI_VERSION == 6 == lib.ygz_hip_abi_version() and re.search(r"#define\s+YGZ_HIP_ABI_VERSION\s+6\b", hdr)
    for s in hip_lib.MPA_SYMBOLS:
        assert s in hip_lib.ABI_SYMBOLS and hasattr(lib, s), s
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
    assert re.search(r"#define\s+YGZ_MPA_MAX_POINTS\s+1048576\b", hdr) and hip_lib.MPA_MAX_POINTS == 1048576 == mpa_ref.MAX_POINTS
    assert (mpa_ref.MAX_KEYFRAMES, mpa_ref.MAX_OBS, mpa_ref.MAX_OBS_PER_POINT) == (hip_lib.MAP_MAX_KEYFRAMES, hip_lib.MAP_MAX_OBS, hip_lib.MAP_MAX_OBS_PER_POINT)
    assert hip_lib.MPA_MAX_LEVEL == 30 == mpa_ref.MAX_LEVEL
    internal = open(os.path.join(PKG, "csrc", "ygz_internal.h")).read()
    assert re.search(r"#define\s+YGZ_N_SCRATCH\s+48\b", internal) and "SCR_MPA" not in internal
    for f in os.listdir(os.path.join(PKG, "csrc")):
        if f.endswith(".hip") and f != "mpa.hip":
            text = open(os.path.join(PKG, "csrc", f)).read()
            assert "SCR_MPA" not in text and not re.search(r"ygz_blob_open\(ctx, 47\b", text), f
    for path in NEW_SOURCES:
        code = re.sub(r"//[^\n]*", "", open(path).read())
        assert "getenv" not in code and "environ" not in code, path


def test_attributes_refuse_every_invalid_call_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.mpa_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY

    def call(K=2, P=None, center=((0.0, 0, 0), (1.0, 1, 1)), pw=((0.0, 0, 3), (1.0, 0, 4)), off=(0, 2, 3), kf=(0, 1, 1), level=(0, 1, 2), null=()):
        a = dict(center=np.array(center, np.float64), pw=np.array(pw, np.float64), off=np.array(off, np.int32), kf=np.array(kf, np.int32),
                 level=np.array(level, np.int32))
        P = len(off) - 1 if P is None else P
        o = dict(dmax=np.full(8, 5.0), normal=np.full(24, 5.0), state=np.full(8, 5, np.int32))
        arg = {k: (dp(v) if v.dtype == np.float64 else ip(v)) for k, v in list(a.items()) + list(o.items())}
        for k in null:
            arg[k] = None
        rc = lib.ygz_hip_map_point_attributes(None, K, arg["center"], P, arg["pw"], arg["off"], arg["kf"], arg["level"], arg["dmax"], arg["normal"],
                                              arg["state"])
        assert all((v == 5).all() for v in o.values())                                 # a refused call writes nothing
        return rc
    # 0: a valid call: only the context is missing
    assert call() == INV and call(off=(0, 0, 0), kf=(0,), level=(0,)) == INV and call(level=(-1, 30, -5)) == INV and call(kf=(1, 1, 1)) == INV
    # 1: nulls and counts
    for k in ("center", "pw", "off", "kf", "level", "dmax", "normal", "state"):
        assert call(null=(k,)) == INV, k
    assert call(K=0) == INV and call(K=-1) == INV and call(P=0) == INV and call(P=-2) == INV
    # 2: capacities; the nulls come before them, they come before the offsets are read
    big = hip_lib.MAP_MAX_KEYFRAMES + 1
    assert call(K=big) == CAP and call(K=big, off=(1, 2, 3)) == CAP and call(K=big, null=("state",)) == INV and call(K=big - 1, center=np.zeros((big, 3))) == INV
    assert call(P=hip_lib.MPA_MAX_POINTS + 1) == CAP and call(P=hip_lib.MPA_MAX_POINTS + 1, off=(3, 2, 1)) == CAP
    # 3: offsets
    assert call(off=(1, 2, 3)) == INV and call(off=(0, 3, 2)) == INV
    # 4: the sizes of the lists, before the lists are read
    n = hip_lib.MAP_MAX_OBS_PER_POINT + 1
    assert call(off=(0, n, n), kf=[7] * n, level=[0] * n) == CAP and call(off=(0, n - 1, n - 1), kf=[0] * n, level=[0] * n) == INV
    P = hip_lib.MAP_MAX_OBS // 256 + 1
    off = np.arange(P + 1, dtype=np.int32) * 256
    assert call(P=P, pw=np.ones((P, 3)), off=off, kf=np.full(off[-1], 9, np.int32), level=np.zeros(off[-1], np.int32)) == CAP
    # 5: indices, levels, finiteness
    assert call(kf=(0, 2, 1)) == INV and call(kf=(-1, 1, 1)) == INV and call(level=(0, 31, 0)) == INV
    assert call(center=((0.0, np.nan, 0), (1.0, 1, 1))) == INV and call(pw=((0.0, 0, 3), (np.inf, 0, 4))) == INV


def test_indexed_call_refuses_every_invalid_call_with_a_null_context(hip_lib):
    lib = hip_lib.load()
    hip_lib.slm_indexed_argtypes(lib)
    hip_lib.slm_argtypes(lib)
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    I = (0.0, 0, 0, 1, 0, 0, 0)

    def params(**kw):
        p = hip_lib.SlmParams()
        lib.ygz_hip_default_slm_params(ctypes.byref(p))
        for k, v in kw.items():
            getattr(p, k)
            setattr(p, k, v)
        return p

    def call(P=3, pw=None, dmax=(1.0, 2, 3), normal=None, lists=((0, 1, 2, 0),), stride=None, length=(3,), n_lists=None, slot=(0,), li=(0,), T=(I,), F=None,
             p=None, null=()):
        a = dict(pw=np.array(np.ones((3, 3)) if pw is None else pw, np.float64), desc=np.zeros((3, 32), np.uint8), dmax=np.array(dmax, np.float64),
                 normal=np.array(np.ones((3, 3)) if normal is None else normal, np.float64), lists=np.array(lists, np.int32),
                 length=np.array(length, np.int32), slot=np.array(slot, np.int32), li=np.array(li, np.int32), T=np.array(T, np.float64))
        stride = a["lists"].shape[-1] if stride is None else stride
        n_lists = len(a["length"]) if n_lists is None else n_lists
        F = len(a["slot"]) if F is None else F
        o = dict(T_out=np.full(64, 5.0), status=np.full(64, 5, np.int32), counts=np.full(64, 5, np.int32))
        conv = lambda v: dp(v) if v.dtype == np.float64 else (bp(v) if v.dtype == np.uint8 else ip(v))
        arg = {k: conv(v) for k, v in list(a.items()) + list(o.items())}
        for k in null:
            arg[k] = None
        rc = lib.ygz_hip_stereo_local_map_indexed(None, P, arg["pw"], arg["desc"], arg["dmax"], arg["normal"], n_lists, stride, arg["lists"], arg["length"],
                                                  F, arg["slot"], arg["li"], arg["T"], None, None if p is None else ctypes.byref(p), arg["T_out"],
                                                  arg["status"], arg["counts"], *([None] * 18))
        assert all((v == 5).all() for v in o.values())                                 # a refused call writes nothing
        return rc
    # 0: a valid call: only the context is missing; a map of no point with an empty list is one too
    assert call() == INV and call(p=params()) == INV and call(P=0, length=(0,), null=("pw", "desc", "dmax", "normal")) == INV
    assert call(null=("status",)) == INV and call(null=("counts",)) == INV
    # 1: nulls and counts
    for k in ("lists", "length", "slot", "li", "T", "T_out"):
        assert call(null=(k,)) == INV, k
    assert call(F=0) == INV and call(F=-1) == INV and call(n_lists=0) == INV and call(P=-1) == INV
    # 2: capacities, before the parameters; the nulls come before them
    n = hip_lib.SLM_MAX_FRAMES + 1
    assert call(F=n) == CAP and call(F=n, p=params(th=0.0)) == CAP and call(F=n, null=("T",)) == INV
    assert call(n_lists=n) == CAP and call(n_lists=65, lists=np.zeros((65, 4)), length=[3] * 65) == INV      # 64 sets are no limit here
    assert call(P=hip_lib.MPA_MAX_POINTS + 1) == CAP and call(P=hip_lib.MPA_MAX_POINTS + 1, p=params(ratio=-1.0)) == CAP
    # 3: parameters, before the map and the lists are looked at
    for bad in (dict(baseline=0.0), dict(th=float("nan")), dict(th_dist=257), dict(min_edges=-1), dict(r_near=0.0)):
        assert call(p=params(**bad)) == INV and call(p=params(**bad), stride=0) == INV, bad
    # 4: the map and the lists
    for k in ("pw", "desc", "dmax", "normal"):
        assert call(null=(k,)) == INV, k
    assert call(stride=0) == INV and call(stride=-4) == INV and call(length=(5,)) == INV and call(length=(-1,)) == INV and call(length=(4,)) == INV
    assert call(slot=(-1,)) == INV and call(li=(1,)) == INV and call(li=(-1,)) == INV
    assert call(lists=((0, 3, 2, 0),)) == INV and call(lists=((0, -1, 2, 0),)) == INV
    assert call(lists=((0, 1, 2, 99),)) == INV                                        # past list_len: not read, the context alone is missing
    assert call(lists=((0, 1, 2, 0), (9, 9, 9, 9)), length=(3, 4)) == INV              # a list no frame reads: not checked
    # 5: the pairs come before the finiteness of anything; 6: finiteness over the whole map, named by a list or not
    F = 1024
    long = np.zeros((1, hip_lib.SLM_MAX_PAIRS // F + 1), np.int32)
    many = dict(lists=long, slot=[0] * F, li=[0] * F, T=[I] * F)
    bad_T = [I] * (F - 1) + [(0.0, 0, 0, 1, np.inf, 0, 0)]
    assert call(length=(long.shape[1],), **many) == CAP and call(length=(long.shape[1],), **dict(many, T=bad_T)) == CAP
    assert call(length=(long.shape[1] - 1,), **dict(many, T=bad_T)) == INV
    nan = np.ones((3, 3))
    nan[2, 1] = np.nan
    assert call(T=((0.0, 0, 0, 1, np.nan, 0, 0),)) == INV and call(pw=nan) == INV and call(normal=nan) == INV and call(dmax=(1.0, np.inf, 3)) == INV
    assert call(pw=nan, lists=((0, 1, 0, 0),)) == INV                                  # point 2 is in no list
