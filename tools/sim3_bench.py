#!/usr/bin/env python3
"""Call time of ygz_hip_sim3_ransac (the loop detection's Sim3 RANSAC and 7-dof refinement, csrc/sim3.hip) beside its restatement on one
host core (tests/sim3_ref.c, gcc -O2), on the same inputs: seeded scenes (depth 2-6 m, noise 0.5 px per level, 30 % outliers) at N = 100,
1000, 3072 per problem, 300 iterations, 1 and 5 problems per call; per row whether every output is bit-identical.  Device: a host clock
around each call, which ends in its one wait; 5 warm-up calls, then 50 timed; median / p10 / p90.  Then the DetectLoop + ComputeSim3 wall
times of the loop scene of tests/test_gpu_loop_closing.py.
Usage (on the GPU box): tools/sim3_bench.py [libloop_surface.so, "" to build one, or - to skip the loop scene] [out.json]; the default
output is profiles/sim3_bench.json."""
import datetime
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_ref as sr                         # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402

FIELDS = ["success", "n_hypotheses", "best_sample", "n_inliers", "n_refined", "lm_iterations", "S12", "S21", "chi2_ransac", "chi2_refined"]


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def main():
    arg = sys.argv[1] if len(sys.argv) > 1 else ""
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "sim3_bench.json")
    so = None if arg == "-" else arg
    if not so and arg != "-":
        from test_loop_surface_build import build_program
        so = build_program(tempfile.mkdtemp(prefix="sim3_bench_"))
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    rows = []
    for n in (100, 1000, 3072):
        for P in (1, 5):
            scs = [sr.scene(n, 3000 + 13 * n + p, noise=0.5, outliers=0.3) for p in range(P)]
            cat = lambda k: np.concatenate([s[k] for s in scs])
            off = np.arange(P + 1) * n
            dev = []
            for k in range(55):
                t0 = time.perf_counter()
                res, mask = ctx.sim3_ransac(cat("X1"), cat("X2"), cat("px1"), cat("px2"), cat("levels"), off, sr.K4_DEFAULT)
                t1 = time.perf_counter()
                if k >= 5:
                    dev.append(t1 - t0)
            host, reps = [], 4 if n == 3072 else 8
            for k in range(reps):
                t0 = time.perf_counter()
                refs = [sr.ransac(s) for s in scs]
                t1 = time.perf_counter()
                if k >= 2:
                    host.append(t1 - t0)
            same = all(all(np.array_equal(np.asarray(res[p][f]), np.asarray(refs[p]["result"][f])) for f in FIELDS)
                       and np.array_equal(mask[off[p]:off[p + 1]], refs[p]["mask"]) for p in range(P))
            row = dict(n=n, problems=P, success=[int(r["success"]) for r in res], refined=[int(r["n_refined"]) for r in res], device=stats(dev),
                       host_one_core=stats(host), bit_identical=bool(same))
            row["speedup_median"] = row["host_one_core"]["median_ms"] / row["device"]["median_ms"]
            rows.append(row)
            print(json.dumps(row))
    ctx.close()
    loop = None
    if so:
        d = tempfile.mkdtemp(prefix="sim3_bench_")
        z = os.path.join(d, "loop.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "loop_driver.py"), so, z], capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            o = np.load(z)["out"]
            loop = dict(note="per keyframe of the loop scene (revisit run, then another texture): host clock around DetectLoop and around "
                             "ComputeSim3 (SearchByBoW per candidate, one ygz_hip_sim3_ransac); 0 when ComputeSim3 was not called",
                        detect_ms=[float(v) for v in o[:, 27]], compute_sim3_ms=[float(v) for v in o[:, 28]], detected=[int(v) for v in o[:, 0]],
                        accepted=[int(v) for v in o[:, 1]], refined_inliers=[int(v) for v in o[:, 25]])
            print(json.dumps(loop))
        else:
            loop = dict(error=r.stderr[-2000:])
    res = dict(note="ygz_hip_sim3_ransac call time (host clock around a call that ends in its wait; 5 warm-up + 50 timed) beside the restatement "
                    "tests/sim3_ref.c on one host core (2 warm-up + 2 or 6 timed); noise 0.5 px per level, 30 % outliers, max_iter 300",
               box=dict(device=device_name(), host_cpu=platform.processor() or platform.machine()),
               date=datetime.date.today().isoformat(), rows=rows, loop=loop)
    json.dump(res, open(out, "w"), indent=1)
    if not all(r["bit_identical"] for r in rows):
        sys.exit(1)


if __name__ == "__main__":
    main()
