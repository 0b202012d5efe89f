#!/usr/bin/env python3
"""Call time of ygz_hip_initialize (the monocular Initializer, csrc/init.hip) beside the restatement of Initializer.cpp on one host core
(tests/init_ref.c, gcc -O2), on the same inputs: seeded general scenes (depth 2-6 m, noise 0.5 px, 10 % outliers) at N = 200, 1000, 3072.
Device: a host clock around each call, which ends in its one wait; 5 warm-up calls, then 50 timed; median / p10 / p90.
Usage (on the GPU box): tools/init_bench.py [out.json]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import init_ref as ir                         # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    rows = []
    for n in (200, 1000, 3072):
        s = ir.scene(n, 1000 + n, noise=0.5, outliers=0.1)
        dev = []
        for k in range(55):
            t0 = time.perf_counter()
            g = ctx.initialize(s["px1"], s["px2"], s["K4"])
            t1 = time.perf_counter()
            if k >= 5:
                dev.append(t1 - t0)
        host = []
        for k in range(12):
            t0 = time.perf_counter()
            r = ir.initialize(s["px1"], s["px2"], s["K4"])
            t1 = time.perf_counter()
            if k >= 2:
                host.append(t1 - t0)
        same = bool(g["success"] == r["result"]["success"] and np.array_equal(g["R21"], r["result"]["R21"]) and np.array_equal(g["pts3d"], r["pts3d"]))
        row = dict(n=n, success=int(g["success"]), model=int(g["model"]), device=stats(dev), host_one_core=stats(host), bit_identical=same)
        row["speedup_median"] = row["host_one_core"]["median_ms"] / row["device"]["median_ms"]
        rows.append(row)
        print(json.dumps(row))
    ctx.close()
    res = dict(note="ygz_hip_initialize call time (host clock around a call that ends in its wait; 5 warm-up + 50 timed) beside the restatement "
                    "tests/init_ref.c on one host core (2 warm-up + 10 timed); general scenes, noise 0.5 px, 10 % outliers, max_iter 200", rows=rows)
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
