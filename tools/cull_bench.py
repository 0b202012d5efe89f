#!/usr/bin/env python3
"""Call time of ygz_hip_keyframe_redundancy and ygz_hip_cull_keyframes (keyframe culling, csrc/cull.hip) beside their restatement on one host
core (tests/cull_ref.c, gcc -O2) on the same arrays, with a bit-identity flag per row.  One local-mapping size -- 20, 40 and 80 candidates
of about 1000 observations among 100 keyframes -- and two whole-map sizes, 1024 and 4096 keyframes, every keyframe a candidate in a shuffled
order.  Observation counts are 1 + Poisson(mean - 1); the keyframes of a point are a run of consecutive indices round a random centre, as
covisible keyframes are; levels are uniform in [0, 8).  The default parameters.  Device: a host clock around each C ABI call, which ends in
its one wait (the arrays are marshalled once, outside the clock); 5 warm-up calls, then 50 timed; median / p10 / p90.  Restatement: the
median of 3 runs (one run where it takes more than 2 s), for the walk in both its forms: cr_cull, which visits every point per candidate, and
cr_cull_indexed, which builds the keyframe-major index a host implementation would.  Usage (on the GPU box): tools/cull_bench.py [out.json];
the default output is profiles/cull_bench.json."""
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
import cull_ref as cr                         # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402

# (name, points, mean observations per point, keyframes, candidates)
ROWS = [("local_mapping", 16000, 6.5, 100, 20), ("local_mapping", 16000, 6.5, 100, 40), ("local_mapping", 16000, 6.5, 100, 80),
        ("whole_map", 150000, 6.5, 1024, 1024), ("whole_map", 150000, 6.5, 4096, 4096)]


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def case(rng, n_points, mean, K):
    n = np.clip(1 + rng.poisson(max(mean - 1.0, 0.0), n_points), 1, min(K, _lib.MAP_MAX_OBS_PER_POINT)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    start = rng.integers(0, K - n + 1)
    kf = (np.repeat(start, n) + np.arange(off[-1]) - np.repeat(off[:-1], n)).astype(np.int32)
    level = rng.integers(0, 8, len(kf)).astype(np.int32)
    return off, kf, level


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
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cull_bench.json")
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    lib = ctx.lib
    _lib.cull_argtypes(lib)
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    P = lambda a, t=ip: a.ctypes.data_as(t)
    rng = np.random.default_rng(17)
    cr.lib()
    rows = []
    for name, n_points, mean, K, n_cand in ROWS:
        off, kf, level = case(rng, n_points, mean, K)
        assert off[-1] <= _lib.MAP_MAX_OBS
        cand = rng.permutation(K)[:n_cand].astype(np.int32)
        t, r = np.zeros(K, np.int32), np.zeros(K, np.int32)
        dev_counts = timed(lambda: lib.ygz_hip_keyframe_redundancy(ctx._ctx, n_points, P(off), P(kf), P(level), K, None, P(t), P(r)))
        counts_ms, ref = host_median(lambda: cr.redundancy(off, kf, level, K))
        same_counts = np.array_equal(ref["tracked"], t) and np.array_equal(ref["redundant"], r)
        c, ct, crd, dead = np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32), np.zeros(n_points, np.uint8)
        dev_walk = timed(lambda: lib.ygz_hip_cull_keyframes(ctx._ctx, n_points, P(off), P(kf), P(level), K, n_cand, P(cand), None, P(c), P(ct),
                                                            P(crd), P(dead, bp)))
        walk_ms, ref = host_median(lambda: cr.cull(off, kf, level, K, cand))
        indexed_ms, ref2 = host_median(lambda: cr.cull(off, kf, level, K, cand, indexed=True))
        same_walk = all(np.array_equal(a[k], b) for a in (ref, ref2) for k, b in [("culled", c), ("tracked", ct), ("redundant", crd), ("point_dead", dead)])
        row = dict(size=name, points=n_points, mean_observations=mean, observations=int(off[-1]), keyframes=K, candidates=n_cand,
                   observations_per_keyframe=float(off[-1]) / K, culled=int(c.sum()), points_dead=int(dead.sum()),
                   redundancy=dict(device=stats(dev_counts), one_core_ms=counts_ms, bit_identical=bool(same_counts)),
                   walk=dict(device=stats(dev_walk), one_core_ms=walk_ms, one_core_indexed_ms=indexed_ms, bit_identical=bool(same_walk)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/cull_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               warmup=5, timed=50, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
