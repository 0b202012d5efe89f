"""ctypes loader of tests/map_ref.c, the restatement of the map-upkeep calls (ygz_slam_amd/csrc/map.hip) that tests/test_map_ref.py holds to
numpy witnesses and tests/test_gpu_map.py holds ygz_hip_distinctive_descriptors / ygz_hip_covisibility against.  Test infrastructure: compiled
with gcc into a temporary directory the first time it is used, never imported by the package.  Also the seeded case generators both tests
share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="map_ref_")
        so = os.path.join(d, "libmap_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "map_ref.c")])
        _lib = ctypes.CDLL(so)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def distinctive(offsets, desc):
    """mr_distinctive: dict(best [P], median [P], desc [P][32])"""
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    P = len(off) - 1
    assert P >= 1 and off[-1] == len(d)
    d = d if len(d) else np.zeros((1, 32), np.uint8)
    best, med, out = np.full(P, -2, np.int32), np.full(P, -2, np.int32), np.full((P, 32), 0xAA, np.uint8)
    lib().mr_distinctive(P, _p(off, ctypes.c_int32), _p(d, ctypes.c_uint8), _p(best, ctypes.c_int32), _p(med, ctypes.c_int32),
                         _p(out, ctypes.c_uint8))
    return dict(best=best, median=med, desc=out)


def covisibility(offsets, kf, K, rows):
    """mr_covisibility: weights [R][K]"""
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    k = np.ascontiguousarray(kf, np.int32).reshape(-1)
    r = np.ascontiguousarray(rows, np.int32).reshape(-1)
    P = len(off) - 1
    assert P >= 1 and off[-1] == len(k)
    k = k if len(k) else np.zeros(1, np.int32)
    w = np.full((len(r), K), -2, np.int32)
    lib().mr_covisibility(P, _p(off, ctypes.c_int32), _p(k, ctypes.c_int32), int(K), len(r), _p(r, ctypes.c_int32), _p(w, ctypes.c_int32))
    return w


# ---- descriptor cases: name -> (offsets [P + 1], desc [n_obs][32])

def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _random_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _clustered(rng, n, max_flips=70):
    """a base descriptor with 0 .. max_flips flipped bits per observation: distances are small and medians tie"""
    base = np.unpackbits(_random_desc(rng, 1)[0])
    out = np.zeros((n, 32), np.uint8)
    for i in range(n):
        bits = base.copy()
        flip = rng.choice(256, int(rng.integers(0, max_flips + 1)), replace=False)
        bits[flip] ^= 1
        out[i] = np.packbits(bits)
    return out


def descriptor_cases():
    rng = np.random.default_rng(1407)
    cases = {}
    for n in [0, 1, 2, 3, 4, 5]:
        cases["n%d" % n] = (_offsets([n]), _random_desc(rng, n))
    cases["small_batch"] = (_offsets([0, 1, 2, 3, 4, 5, 0, 2]), _random_desc(rng, 17))
    cases["identical"] = (_offsets([7, 4]), np.repeat(_random_desc(rng, 1), 11, axis=0))
    counts = [9, 6, 12, 5, 8]
    cases["clustered"] = (_offsets(counts), np.concatenate([_clustered(rng, c) for c in counts]))
    cases["clustered_tight"] = (_offsets([10, 7]), np.concatenate([_clustered(rng, 10, 3), _clustered(rng, 7, 2)]))
    for n in [63, 64, 65, 255, 256]:
        cases["n%d" % n] = (_offsets([n]), _clustered(rng, n) if n % 2 else _random_desc(rng, n))
    counts = rng.integers(1, 13, 300)
    cases["batch300"] = (_offsets(counts), np.concatenate([_clustered(rng, c) if i % 3 else _random_desc(rng, c) for i, c in enumerate(counts)]))
    return cases


# ---- weight cases: name -> (offsets [P + 1], kf [n_obs], K, rows [R])

def _lists(rng, n_points, K, lo, hi, always=None):
    lists = []
    for _ in range(n_points):
        n = int(rng.integers(lo, min(hi, K) + 1))
        l = set(int(v) for v in rng.choice(K, n, replace=False)) if n else set()
        if always is not None:
            l.add(always)
        lists.append(sorted(l))
    return lists


def _pack(lists):
    off = _offsets([len(l) for l in lists])
    kf = np.array([k for l in lists for k in l], np.int32)
    return off, kf


HAND_K5 = dict(lists=[[0, 1, 2], [1, 2], [2, 4], [], [0, 2, 3, 4], [1]], rows=[2, 0, 4],
               weights=[[2, 2, 4, 1, 2], [2, 1, 2, 1, 1], [1, 0, 2, 1, 2]])


def weight_cases():
    rng = np.random.default_rng(2203)
    cases = {}
    cases["k1"] = _pack([[0], [0], [], [0]]) + (1, np.array([0], np.int32))
    cases["k2"] = _pack([[0, 1], [1], [0], [0, 1], []]) + (2, np.array([1, 0], np.int32))
    cases["hand_k5"] = _pack(HAND_K5["lists"]) + (5, np.array(HAND_K5["rows"], np.int32))
    l130 = _lists(rng, 700, 130, 1, 12)
    cases["k130_all"] = _pack(l130) + (130, np.arange(130, dtype=np.int32))
    cases["k130_subset"] = _pack(l130) + (130, rng.permutation(130)[:37].astype(np.int32))
    cases["p2000"] = _pack(_lists(rng, 2000, 200, 1, 20)) + (200, rng.permutation(200)[:64].astype(np.int32))
    cases["column0"] = _pack(_lists(rng, 2000, 200, 1, 20, always=0)) + (200, rng.permutation(200).astype(np.int32))
    cases["empties"] = _pack(_lists(rng, 500, 60, 0, 4)) + (60, rng.permutation(60)[:25].astype(np.int32))
    return cases
