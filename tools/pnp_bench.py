#!/usr/bin/env python3
"""Call time of ygz_hip_pnp_ransac (the relocalisation's P3P RANSAC, csrc/pnp.hip) beside its restatement on one host core (tests/pnp_ref.c,
gcc -O2), on the same inputs: seeded general scenes (depth 2-6 m, noise 0.5 px, 30 % outliers) at N = 100, 1000, 3072 per problem, 300
iterations, 1 and 5 problems per call.  Device: a host clock around each call, which ends in its one wait; 5 warm-up calls, then 50 timed;
median / p10 / p90.  Then one ygz::Relocalizer::Relocalize per kidnapped frame on the synthetic map of tests/test_gpu_relocalize.py.
Usage (on the GPU box): tools/pnp_bench.py <libreloc_surface.so or -> [out.json]"""
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
import pnp_ref as pr                          # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402


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
    so = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] != "-" else None
    out = sys.argv[2] if len(sys.argv) > 2 else None
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    rows = []
    for n in (100, 1000, 3072):
        for P in (1, 5):
            scs = [pr.scene(n, 2000 + 13 * n + p, noise=0.5, outliers=0.3) for p in range(P)]
            pw = np.concatenate([s["pw"] for s in scs]); px = np.concatenate([s["px"] for s in scs])
            off = np.arange(P + 1) * n
            dev = []
            for k in range(55):
                t0 = time.perf_counter()
                res, inl = ctx.pnp_ransac(pw, px, off, pr.K4_DEFAULT)
                t1 = time.perf_counter()
                if k >= 5:
                    dev.append(t1 - t0)
            host, reps = [], 6 if n == 3072 else 12
            for k in range(reps):
                t0 = time.perf_counter()
                refs = [pr.ransac(s["pw"], s["px"], pr.K4_DEFAULT) for s in scs]
                t1 = time.perf_counter()
                if k >= 2:
                    host.append(t1 - t0)
            same = all(res[p]["n_inliers"] == refs[p]["result"]["n_inliers"] and np.array_equal(res[p]["T_cw"], refs[p]["result"]["T_cw"])
                       and np.array_equal(inl[off[p]:off[p + 1]], refs[p]["inliers"]) for p in range(P))
            row = dict(n=n, problems=P, success=[int(r["success"]) for r in res], device=stats(dev), host_one_core=stats(host), bit_identical=same)
            row["speedup_median"] = row["host_one_core"]["median_ms"] / row["device"]["median_ms"]
            rows.append(row)
            print(json.dumps(row))
    ctx.close()
    reloc = None
    if so:
        d = tempfile.mkdtemp(prefix="pnp_bench_")
        z = os.path.join(d, "reloc.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reloc_driver.py"), so, z], capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            o = np.load(z)["out"]
            reloc = dict(note="one Relocalizer::Relocalize per frame (host clock around the call: extraction, BoW, retrieval, SearchByBoW, one "
                              "ygz_hip_pnp_ransac, pose-only BA); 5 keyframes, kidnapped frames of the same trajectory then one unseen frame",
                         ms=[float(v) for v in o[:, 26]], ok=[int(v) for v in o[:, 0]], ransac_inliers=[int(v) for v in o[:, 10]],
                         final_inliers=[int(v) for v in o[:, 11]], candidates=[int(v) for v in o[:, 8]])
            print(json.dumps(reloc))
        else:
            reloc = dict(error=r.stderr[-2000:])
    res = dict(note="ygz_hip_pnp_ransac call time (host clock around a call that ends in its wait; 5 warm-up + 50 timed) beside the restatement "
                    "tests/pnp_ref.c on one host core (2 warm-up + 4 or 10 timed); general scenes, noise 0.5 px, 30 % outliers, max_iter 300",
               box=dict(device=device_name(), host_cpu=platform.processor() or platform.machine()),
               date=datetime.date.today().isoformat(), rows=rows, relocalize=reloc)
    if out:
        json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    main()
