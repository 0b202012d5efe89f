#!/usr/bin/env python3
"""Call time of ygz_hip_global_ba (the global bundle adjustment, csrc/gba.hip) beside two yardsticks on the same problems: its restatement on
one host core (tests/gba_ref.c, gcc -O2), and ygz_hip_ba_optimize, the library's only other way to do this job, whose host-loop path takes over
above 20 free poses (the GPU linearises, a dense reduced system is solved on the host, every trial crosses PCIe); that one retracts by g2o's
exponential, so the two agree at convergence, not bit for bit, and its final cost is recorded beside the solver's.  Problems: tests/gba_ref.py's
rings of cameras around a point cloud, N = 16, 128 and 512 poses, 16 N points of 8 observations each (128 per pose), pixel noise 0.5,
perturbed starts.  Per row: whether the device is bit-identical to the restatement, the LM iterations, the solves and the CG iterations per
solve.  Device: a host clock around each C ABI call, which ends in its wait (the arrays are marshalled once, outside the clock); 5 warm-up
calls, then 50 timed (fewer when 50 would take more than a minute, never fewer than 5); median / p10 / p90.  Restatement: the median of 3 runs
(1 run at N = 512).  ygz_hip_ba_optimize: one warm-up call, then the median of 3 (1 at N = 512).  Usage (on the GPU box): tools/gba_bench.py
[out.json]; the default output is profiles/gba_bench.json."""
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
import gba_ref as gb                          # noqa: E402  (test infrastructure: the one-core restatement and the scenes)
from ygz_slam_amd import _lib                 # noqa: E402

SIZES = (16, 128, 512)
POINTS_PER_POSE, OBS_PER_POINT = 16, 8


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def se3_log(T):
    """(q, t) -> ygz_ba_problem's pose [omega; upsilon] with exp([upsilon; omega]) = (R, t)"""
    q = np.asarray(T[:4], float)
    q = q / np.linalg.norm(q)
    if q[3] < 0:
        q = -q
    s = np.linalg.norm(q[:3])
    th = 2 * np.arctan2(s, q[3])
    w = q[:3] / s * th if s > 1e-12 else 2 * q[:3]
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    V = np.eye(3) + ((1 - np.cos(th)) / th ** 2 * W + (th - np.sin(th)) / th ** 3 * W @ W if th > 1e-8 else 0.5 * W)
    return np.concatenate([w, np.linalg.solve(V, np.asarray(T[4:], float))])


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gba_bench.json")
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    lib = ctx.lib
    _lib.gba_argtypes(lib)
    prm = _lib.default_gba_params()
    rows = []
    for n in SIZES:
        g = gb.scene(n, POINTS_PER_POSE * n, OBS_PER_POINT, noise=0.5, seed=n, rings=max(1, n // 64))
        poses, fixed, points, ep, el, obs = _lib.gba_arrays(g["poses"], g["fixed"], g["points"], g["edge_pose"], g["edge_point"], g["obs"])
        K = np.ascontiguousarray(g["K"], np.float64)
        po, xo, res = np.zeros_like(poses), np.zeros_like(points), _lib.GbaResult()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        args = (ctx._ctx, len(poses), poses.ctypes.data_as(dp), fixed.ctypes.data_as(C.POINTER(C.c_uint8)), len(points), points.ctypes.data_as(dp),
                len(ep), ep.ctypes.data_as(ip), el.ctypes.data_as(ip), obs.ctypes.data_as(dp), K.ctypes.data_as(dp), float(g["huber"]), C.byref(prm),
                po.ctypes.data_as(dp), xo.ctypes.data_as(dp), C.byref(res))
        dev, spent = [], 0.0
        for k in range(55):
            t0 = time.perf_counter()
            rc = lib.ygz_hip_global_ba(*args)
            t1 = time.perf_counter()
            assert rc == 0, rc
            if k >= 5:
                dev.append(t1 - t0)
                spent += t1 - t0
                if spent > 60.0 and len(dev) >= 5:
                    break
        host = []
        for k in range(1 if n >= 512 else 3):
            t0 = time.perf_counter()
            ref = gb.optimize(g)
            host.append(time.perf_counter() - t0)
        same = np.array_equal(ref["poses"].view(np.uint64), po.view(np.uint64)) and np.array_equal(ref["points"].view(np.uint64), xo.view(np.uint64)) \
            and all(getattr(res, k) == ref[k] for k in gb.RESULT_FIELDS)
        row = dict(poses=n, points=len(points), edges=len(ep), unknowns=6 * int((fixed == 0).sum()) + 3 * len(points), device=stats(dev),
                   one_core_ms=float(np.median(host) * 1e3), bit_identical=bool(same), status=res.status, lm_iterations=res.lm_iterations,
                   solves=res.n_solves, cg_iterations=res.cg_iterations_total, cg_capped=res.cg_capped,
                   cg_per_solve=res.cg_iterations_total / max(res.n_solves, 1), cost_initial=res.cost_initial, cost_final=res.cost_final)
        row["device_us_per_cg_iteration"] = 1e3 * row["device"]["median_ms"] / max(res.cg_iterations_total, 1)
        row["one_core_over_device"] = row["one_core_ms"] / row["device"]["median_ms"]
        # the library's other way: ygz_hip_ba_optimize (formulation 0, the same edge model), 10 iterations like the solver
        try:
            p6 = np.array([se3_log(T) for T in poses])
            cam = tuple(float(v) for v in g["K"])
            old = []
            for k in range(2 if n >= 512 else 4):
                t0 = time.perf_counter()
                _, _, st = ctx.ba_optimize(p6, fixed, points, ep, el, obs, iterations=prm.max_iterations, huber_delta=float(g["huber"]), cam=cam)
                if k:
                    old.append(time.perf_counter() - t0)
            resident, why = ctx.ba_last_path()
            row["ba_optimize"] = dict(median_ms=float(np.median(old) * 1e3), calls=len(old), path="resident" if resident else "host loop",
                                      reasons=why, iterations=st.iterations, lm_trials=st.lm_trials, cost_initial=st.chi2_initial,
                                      cost_final=st.chi2_final)
            row["ba_optimize_over_device"] = row["ba_optimize"]["median_ms"] / row["device"]["median_ms"]
        except Exception as e:                # noqa: BLE001  (a refusal of the other entry point is a result, not a failure of this tool)
            row["ba_optimize"] = dict(error=str(e))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/gba_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               params=dict(max_iterations=prm.max_iterations, max_trials=prm.max_trials, cg_max_iterations=prm.cg_max_iterations, cg_batch=prm.cg_batch,
                           cg_tol=prm.cg_tol, min_rel_decrease=prm.min_rel_decrease, huber_delta=gb.HUBER),
               scene=dict(points_per_pose=POINTS_PER_POSE, observations_per_point=OBS_PER_POINT, pixel_noise=0.5), warmup=5, timed=50, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
