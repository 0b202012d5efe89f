#!/usr/bin/env python3
"""Call time of ygz_hip_distinctive_descriptors and ygz_hip_covisibility (the map upkeep of loop fusion, csrc/map.hip) beside their restatement
on one host core (tests/map_ref.c, gcc -O2) on the same arrays, with a bit-identity flag per row.  A sweep over the point count, the mean
number of observations per point and the keyframe count that includes the loop scene's sizes (tests/test_gpu_loop_fuse.py: about 1500 loop
map points of 2-6 observations; 17 keyframes and 17 000 points of mostly one observation).  Observation counts are 1 + Poisson(mean - 1),
cut at the call's limit; descriptors are a base per point with 0-70 flipped bits; keyframes of a point are a run of consecutive indices round
a random centre, as covisible keyframes are.  Device: a host clock around each C ABI call, which ends in its one wait (the arrays are
marshalled once, outside the clock); 5 warm-up calls, then 50 timed; median / p10 / p90.  Restatement: the median of 3 runs (one run where it takes more than 2 s).  Usage (on the GPU
box): tools/map_bench.py [out.json]; the default output is profiles/map_bench.json."""
import ctypes as C
import datetime
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_ref as mr                          # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402

# (points, mean observations per point); the first is the loop scene's
DESCRIPTOR_ROWS = [(1500, 3), (10000, 4), (100000, 4), (100000, 8), (2000, 64), (1000, 200)]
# (points, mean observations, keyframes, rows); the first is the loop scene's
WEIGHT_ROWS = [(17000, 1.2, 17, 17), (20000, 4, 128, 128), (20000, 4, 128, 16), (100000, 6, 1024, 1024), (100000, 6, 1024, 32),
               (150000, 6, 4096, 1024)]


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def counts(rng, n_points, mean, cap):
    return np.clip(1 + rng.poisson(max(mean - 1.0, 0.0), n_points), 1, cap).astype(np.int64)


def descriptor_case(rng, n_points, mean):
    n = counts(rng, n_points, mean, _lib.MAP_MAX_OBS_PER_POINT)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    base = np.repeat(rng.integers(0, 256, (n_points, 32), dtype=np.uint8), n, axis=0)
    flips = rng.integers(0, 256, (len(base), 256), dtype=np.uint8) < rng.integers(0, 71, len(base)).astype(np.uint8)[:, None]
    return off, base ^ np.packbits(flips, axis=1)


def weight_case(rng, n_points, mean, K):
    n = counts(rng, n_points, mean, K)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    start = np.array([rng.integers(0, K - c + 1) for c in n])
    kf = np.concatenate([np.arange(s, s + c) for s, c in zip(start, n)]).astype(np.int32)
    return off, kf


def timed(call, warmup=5, n=50):
    ts = []
    for k in range(warmup + n):
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        assert rc == 0, rc
        if k >= warmup:
            ts.append(t1 - t0)
    return ts


def host_median(f, runs=3):
    ts, r = [], None
    for _ in range(runs):
        t0 = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t0)
        if ts[-1] > 2.0:                      # one run of a slow row
            break
    return float(np.median(ts) * 1e3), r


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "map_bench.json")
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    lib = ctx.lib
    _lib.map_argtypes(lib)
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rng = np.random.default_rng(14)
    mr.lib()
    drows, wrows = [], []
    for n_points, mean in DESCRIPTOR_ROWS:
        off, desc = descriptor_case(rng, n_points, mean)
        best, med, od = np.zeros(n_points, np.int32), np.zeros(n_points, np.int32), np.zeros((n_points, 32), np.uint8)
        dev = timed(lambda: lib.ygz_hip_distinctive_descriptors(ctx._ctx, n_points, off.ctypes.data_as(ip), desc.ctypes.data_as(bp),
                                                                best.ctypes.data_as(ip), med.ctypes.data_as(ip), od.ctypes.data_as(bp)))
        host_ms, ref = host_median(lambda: mr.distinctive(off, desc))
        same = np.array_equal(ref["best"], best) and np.array_equal(ref["median"], med) and np.array_equal(ref["desc"], od)
        row = dict(points=n_points, mean_observations=mean, observations=int(off[-1]), max_observations=int(np.diff(off).max()),
                   device=stats(dev), one_core_ms=host_ms, bit_identical=bool(same))
        row["one_core_over_device"] = row["one_core_ms"] / row["device"]["median_ms"]
        drows.append(row)
        print(json.dumps(row), flush=True)
    for n_points, mean, K, R in WEIGHT_ROWS:
        off, kf = weight_case(rng, n_points, mean, K)
        rows = (np.arange(K) if R == K else rng.permutation(K)[:R]).astype(np.int32)
        w = np.zeros((R, K), np.int32)
        dev = timed(lambda: lib.ygz_hip_covisibility(ctx._ctx, n_points, off.ctypes.data_as(ip), kf.ctypes.data_as(ip), K, R,
                                                     rows.ctypes.data_as(ip), w.ctypes.data_as(ip)))
        host_ms, ref = host_median(lambda: mr.covisibility(off, kf, K, rows))
        row = dict(points=n_points, mean_observations=mean, observations=int(off[-1]), keyframes=K, rows=R, cells=R * K, device=stats(dev),
                   one_core_ms=host_ms, bit_identical=bool(np.array_equal(ref, w)))
        row["one_core_over_device"] = row["one_core_ms"] / row["device"]["median_ms"]
        wrows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/map_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               warmup=5, timed=50, distinctive_descriptors=drows, covisibility=wrows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
