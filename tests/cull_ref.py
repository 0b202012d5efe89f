"""ctypes loader of tests/cull_ref.c, the restatement of the keyframe-culling calls (ygz_slam_amd/csrc/cull.hip) that tests/test_cull_ref.py
holds to a numpy witness and tests/test_gpu_cull.py holds ygz_hip_keyframe_redundancy / ygz_hip_cull_keyframes against.  Test infrastructure:
compiled with gcc into a temporary directory the first time it is used, never imported by the package.  Also the case generators both tests
share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

DEFAULTS = dict(th_obs=3, ratio=0.9, level_slack=-1, min_obs=2)


class Params(ctypes.Structure):
    """cr_params = ygz_cull_params"""
    _fields_ = [("th_obs", ctypes.c_int32), ("level_slack", ctypes.c_int32), ("min_obs", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("ratio", ctypes.c_double)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="cull_ref_")
        so = os.path.join(d, "libcull_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "cull_ref.c")])
        _lib = ctypes.CDLL(so)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(**kw):
    v = dict(DEFAULTS, **kw)
    return Params(int(v["th_obs"]), int(v["level_slack"]), int(v["min_obs"]), 0, float(v["ratio"]))


def _arrays(offsets, kf, level):
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    k = np.ascontiguousarray(kf, np.int32).reshape(-1)
    l = np.ascontiguousarray(level, np.int32).reshape(-1)
    assert len(off) >= 2 and off[-1] == len(k) == len(l)
    if not len(k):
        k, l = np.zeros(1, np.int32), np.zeros(1, np.int32)
    return off, k, l


def redundancy(offsets, kf, level, K, **kw):
    """cr_redundancy: dict(tracked [K], redundant [K])"""
    off, k, l = _arrays(offsets, kf, level)
    q = params(**kw)
    t, r = np.full(K, -2, np.int32), np.full(K, -2, np.int32)
    lib().cr_redundancy(len(off) - 1, _p(off, ctypes.c_int32), _p(k, ctypes.c_int32), _p(l, ctypes.c_int32), int(K), ctypes.byref(q),
                        _p(t, ctypes.c_int32), _p(r, ctypes.c_int32))
    return dict(tracked=t, redundant=r)


def cull(offsets, kf, level, K, cand, indexed=False, **kw):
    """cr_cull (indexed: cr_cull_indexed, the same walk over a keyframe-major index): dict(culled, tracked, redundant [n_cand], point_dead [P])"""
    off, k, l = _arrays(offsets, kf, level)
    c = np.ascontiguousarray(cand, np.int32).reshape(-1)
    q = params(**kw)
    n, P = len(c), len(off) - 1
    o = dict(culled=np.full(n, -2, np.int32), tracked=np.full(n, -2, np.int32), redundant=np.full(n, -2, np.int32),
             point_dead=np.full(P, 0xAA, np.uint8))
    walk = lib().cr_cull_indexed if indexed else lib().cr_cull
    walk(P, _p(off, ctypes.c_int32), _p(k, ctypes.c_int32), _p(l, ctypes.c_int32), int(K), n, _p(c, ctypes.c_int32), ctypes.byref(q),
         _p(o["culled"], ctypes.c_int32), _p(o["tracked"], ctypes.c_int32), _p(o["redundant"], ctypes.c_int32), _p(o["point_dead"], ctypes.c_uint8))
    return o


# ---- cases: name -> dict(off [P + 1], kf [n_obs], level [n_obs], K, params {}, and for a walk cand [n_cand])

def _lists(rng, n_points, K, lo, hi, always=None, pool=None):
    pool = np.arange(K) if pool is None else np.asarray(pool)
    lists = []
    for _ in range(n_points):
        n = int(rng.integers(lo, min(hi, len(pool)) + 1))
        l = set(int(v) for v in rng.choice(pool, n, replace=False)) if n else set()
        if always is not None:
            l.add(always)
        lists.append(sorted(l))
    return lists


def _case(lists, K, levels=None, cand=None, rng=None, **prm):
    """lists of keyframes per point; levels: None (all 0), "random" (needs rng) or lists of the same shape"""
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    kf = np.array([k for l in lists for k in l], np.int32)
    if levels is None:
        level = np.zeros(len(kf), np.int32)
    elif isinstance(levels, str):
        level = rng.integers(0, 8, len(kf)).astype(np.int32)
    else:
        level = np.array([v for l in levels for v in l], np.int32)
    assert len(level) == len(kf) and all(list(l) == sorted(set(l)) for l in lists)
    c = dict(off=off, kf=kf, level=level, K=int(K), params=prm)
    if cand is not None:
        c["cand"] = np.asarray(cand, np.int32)
    return c


# K = 5, every level 0, the default parameters; the numbers are worked out by hand
HAND = dict(lists=[[0, 1, 2, 3], [0, 1, 2], [1, 2, 3, 4], [0, 4], [0, 1, 2, 3, 4], []], K=5,
            tracked=[4, 4, 4, 3, 3], redundant=[2, 3, 3, 3, 2],
            walks=[dict(cand=[3, 1, 0], params={}, culled=[1, 0, 0], tracked=[3, 4, 4], redundant=[3, 1, 1], point_dead=[0, 0, 0, 0, 0, 0]),
                   dict(cand=[4, 0], params=dict(ratio=0.6), culled=[1, 1], tracked=[3, 3], redundant=[2, 2], point_dead=[0, 0, 0, 1, 0, 0])])


def count_cases():
    rng = np.random.default_rng(1709)
    cases = {}
    cases["hand_k5"] = _case(HAND["lists"], HAND["K"])
    cases["obs0to5"] = _case([list(range(n)) for n in range(6)] + [[5], [2, 5], []], 6)
    # keyframe 0 with exactly th_obs - 1, th_obs and th_obs + 1 other observers, for th_obs 1, 3 and 5
    for th in [1, 3, 5]:
        cases["th%d_edge" % th] = _case([list(range(n + 1)) for n in (th - 1, th, th + 1)] * 3, th + 2, th_obs=th)
    # keyframe 0 at level 2, the others at level 2 + slack and 2 + slack + 1: the first kind counts, the second does not
    for slack in [0, 1]:
        lists = [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3, 4]]
        lv = [[2, 2 + slack, 2 + slack, 2 + slack], [2, 2 + slack, 2 + slack, 3 + slack], [2, 3 + slack, 2 + slack, 0, 2 + slack]]
        cases["level_edge_slack%d" % slack] = _case(lists, 5, levels=lv, level_slack=slack)
    l40 = _lists(rng, 400, 40, 1, 9)
    lv40 = [[int(v) for v in rng.integers(0, 16, len(l))] for l in l40]
    for slack in [-1, 0, 1, 15]:
        cases["levels_slack%d" % slack] = _case(l40, 40, levels=lv40, level_slack=slack)
    for n in [63, 64, 65, 255, 256]:
        lists = [list(range(n))] + _lists(rng, 20, n, 1, 6)
        cases["n%d" % n] = _case(lists, n, levels="random", rng=rng, level_slack=1 if n % 2 else -1)
    cases["batch300"] = _case(_lists(rng, 300, 130, 1, 12), 130)
    cases["k1"] = _case([[0], [0], [], [0]], 1)
    cases["k1_th1"] = _case([[0], [0], [], [0]], 1, th_obs=1)
    cases["k2"] = _case([[0, 1], [1], [0], [0, 1], []], 2, th_obs=1)
    cases["k130"] = _case(_lists(rng, 700, 130, 1, 12), 130, levels="random", rng=rng, level_slack=1)
    # keyframes 7 and 59 see nothing
    cases["without_points"] = _case(_lists(rng, 500, 60, 0, 6, pool=[k for k in range(60) if k not in (7, 59)]), 60)
    cases["column0"] = _case(_lists(rng, 2600, 200, 1, 8, always=0), 200)
    cases["k4096"] = _case(_lists(rng, 3000, 4096, 2, 7), 4096, th_obs=2)
    return cases


def _ratio_edge(n_redundant):
    # keyframe 0 tracks 10 points, n_redundant of them with three more observers
    return [[0, 1, 2, 3]] * n_redundant + [[0, 1]] * (10 - n_redundant)


def _cascade():
    # A = 0, B = 1.  A: 20 points with C, D, E and one shared with B alone.  B: that one and 9 with C, D, E
    return [[0, 2, 3, 4]] * 20 + [[0, 1]] + [[1, 2, 3, 4]] * 9


def walk_cases():
    rng = np.random.default_rng(2311)
    cases = {}
    for i, w in enumerate(HAND["walks"]):
        cases["hand_k5_%d" % i] = _case(HAND["lists"], HAND["K"], cand=w["cand"], **w["params"])
    l130 = _lists(rng, 700, 130, 1, 12)
    lv130 = [[int(v) for v in rng.integers(0, 6, len(l))] for l in l130]
    perm = rng.permutation(130)
    for k in [3, 77, 129]:
        cases["one_kf%d" % k] = _case(l130, 130, cand=[k], ratio=0.93)
    cases["cand64"] = _case(l130, 130, cand=perm[:64], ratio=0.93)
    cases["cand65"] = _case(l130, 130, cand=perm[:65], ratio=0.93, min_obs=3)
    cases["cand_all"] = _case(l130, 130, cand=perm, ratio=0.45)
    cases["cand_all_ascending"] = _case(l130, 130, cand=np.arange(130), ratio=0.45, min_obs=0)
    cases["cand_all_levels"] = _case(l130, 130, levels=lv130, cand=perm[::-1], ratio=0.3, level_slack=1)
    cases["subset"] = _case(l130, 130, levels=lv130, cand=rng.permutation(130)[:37], ratio=0.8, level_slack=0, th_obs=2)
    # keyframe 0 sees nothing, keyframe 1 the first 1025 points, keyframe 2 the first 2500: more observations than the block has lanes
    lists = _lists(rng, 2600, 40, 2, 6, pool=np.arange(3, 40))
    lists = [sorted(l + ([1] if i < 1025 else []) + ([2] if i < 2500 else [])) for i, l in enumerate(lists)]
    for name, cand in [("big_first", [2, 1, 0] + list(range(3, 40))), ("big_last", list(range(39, -1, -1))), ("big_only", [1, 0, 2])]:
        cases[name] = _case(lists, 40, cand=cand, ratio=0.7)
    cases["ratio_9_of_10"] = _case(_ratio_edge(9), 4, cand=[0])
    cases["ratio_10_of_10"] = _case(_ratio_edge(10), 4, cand=[0])
    pair = [[0, 1, 2, 3]] * 12
    cases["order_ab"] = _case(pair, 4, cand=[0, 1])
    cases["order_ba"] = _case(pair, 4, cand=[1, 0])
    for mo in [2, 0]:
        cases["cascade_ab_min%d" % mo] = _case(_cascade(), 5, cand=[0, 1], min_obs=mo)
        cases["cascade_ba_min%d" % mo] = _case(_cascade(), 5, cand=[1, 0], min_obs=mo)
    cases["column0"] = _case(_lists(rng, 2600, 200, 3, 8, always=0), 200, cand=np.arange(200), ratio=0.8)
    cases["empty_lists"] = _case([[], [], []], 3, cand=[2, 0])
    return cases


# what the named walks have to decide, whatever computes them
EXPECTED_CULLED = {"ratio_9_of_10": [0], "ratio_10_of_10": [1], "order_ab": [1, 0], "order_ba": [1, 0], "cascade_ab_min2": [1, 1],
                   "cascade_ba_min2": [0, 1], "cascade_ab_min0": [1, 0], "cascade_ba_min0": [0, 1]}


def run_counts(case, fn=redundancy):
    return fn(case["off"], case["kf"], case["level"], case["K"], **case["params"])


def run_walk(case, fn=cull):
    return fn(case["off"], case["kf"], case["level"], case["K"], case["cand"], **case["params"])
