#!/usr/bin/env python3
"""Call time of ygz_hip_stereo_ba (the stereo bundle adjustment, csrc/sba.hip) with ygz_hip_global_ba beside it on the same problems as the
yardstick.  The two calls do not do the same work -- two rounds of 5 and 10 LM iterations over three-row edges with a classification after
each, against one round of 15 iterations over two-row edges -- so no ratio is a target; both are written down.  Problems: the global bundle
adjustment's rings of cameras around a point cloud (tests/gba_ref.py, tools/gba_bench.py), N = 16, 128 and 512 poses, 16 N points of 8
observations each, with tests/sba_ref.py's levels cycling 0 .. 3, noise 0.5 x 2^level, half the edges stereo and 10 % gross outliers;
default parameters (baseline 0.1).  The yardstick gets the same edges' (u, v) with the Huber width 5.991 and 15 iterations.  A host clock
around each C ABI call, which ends in its wait (the arrays are marshalled once, outside the clock); 5 warm-up calls, then 30 timed; median /
p10 / p90.  Launches: the stereo call reports the kernels it queued (ygz_sba_result::launches); for both calls the same count is also
estimated from the counters alone -- per round 4 (5 with the classification), per solve 3 + ceil(CG iterations per solve / batch) x (3 batch +
8) -- which is what the yardstick's column holds.  Per row also whether the device is bit-identical to the restatement (one host core, run
once).  Usage (on the GPU box): tools/sba_bench.py [out.json]; the default output is profiles/sba_bench.json."""
import ctypes as C
import datetime
import json
import math
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sba_ref as sb                          # noqa: E402  (test infrastructure: the one-core restatement and the scenes)
from ygz_slam_amd import _lib                 # noqa: E402

SIZES = (16, 128, 512)
POINTS_PER_POSE, OBS_PER_POINT = 16, 8
WARMUP, TIMED, BATCH = 5, 30, 8
GBA_ITERATIONS = 15


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def estimate(rounds, per_round, solves, cg):
    return int(rounds * per_round + sum(s * 3 + s * max(1, math.ceil(c / max(s, 1) / BATCH)) * (3 * BATCH + 8) for s, c in zip(solves, cg)))


def timed(call):
    ts = []
    for k in range(WARMUP + TIMED):
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        assert rc == 0, rc
        if k >= WARMUP:
            ts.append(t1 - t0)
    return ts


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sba_bench.json")
    sb.lib()                                  # compiled before any clock starts
    ctx = _lib.HipContext(width=640, height=480, levels=4, max_frames=2)
    lib = ctx.lib
    _lib.sba_argtypes(lib)
    _lib.gba_argtypes(lib)
    prm = _lib._sba_params(baseline=sb.BASELINE)
    gprm = _lib._gba_params(max_iterations=GBA_ITERATIONS)
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    rows = []
    for n in SIZES:
        g = sb.scene(n, POINTS_PER_POSE * n, OBS_PER_POINT, stereo="half", outliers=0.1, seed=n, rings=max(1, n // 64))
        poses, fixed, points, ep, el, obs, kind, level = _lib.sba_arrays(g["poses"], g["fixed"], g["points"], g["edge_pose"], g["edge_point"],
                                                                         g["obs"], g["kind"], g["level"])
        K = np.ascontiguousarray(g["K"], np.float64)
        obs2 = np.ascontiguousarray(obs[:, :2])
        po, xo, res, gres = np.zeros_like(poses), np.zeros_like(points), _lib.SbaResult(), _lib.GbaResult()
        outl, chi2 = np.zeros(len(ep), np.uint8), np.zeros(len(ep))
        head = (ctx._ctx, len(poses), poses.ctypes.data_as(dp), fixed.ctypes.data_as(bp), len(points), points.ctypes.data_as(dp), len(ep),
                ep.ctypes.data_as(ip), el.ctypes.data_as(ip))
        sargs = head + (obs.ctypes.data_as(dp), kind.ctypes.data_as(bp), level.ctypes.data_as(ip), K.ctypes.data_as(dp), C.byref(prm),
                        po.ctypes.data_as(dp), xo.ctypes.data_as(dp), outl.ctypes.data_as(bp), chi2.ctypes.data_as(dp), C.byref(res))
        gargs = head + (obs2.ctypes.data_as(dp), K.ctypes.data_as(dp), 5.991, C.byref(gprm), po.ctypes.data_as(dp), xo.ctypes.data_as(dp), C.byref(gres))
        g_ts = timed(lambda: lib.ygz_hip_global_ba(*gargs))
        s_ts = timed(lambda: lib.ygz_hip_stereo_ba(*sargs))                      # last: po, xo, outl and chi2 hold its answer
        d = res.to_dict()
        t0 = time.perf_counter()
        ref = sb.optimize(g)
        one_core = time.perf_counter() - t0
        same = np.array_equal(ref["poses"].view(np.uint64), po.view(np.uint64)) and np.array_equal(ref["points"].view(np.uint64), xo.view(np.uint64)) \
            and np.array_equal(ref["outlier"], outl) and np.array_equal(ref["chi2"].view(np.uint64), chi2.view(np.uint64)) \
            and all(np.array_equal(np.asarray(ref[k]), np.asarray(d[k])) for k in ("status", "lm_iterations", "n_solves", "cg_iterations", "inliers"))
        r = d["rounds_run"]
        row = dict(poses=n, points=len(points), edges=len(ep), stereo_edges=int((kind == 2).sum()), displaced=int(g["displaced"].sum()),
                   stereo_ba=dict(stats(s_ts), rounds_run=r, status=d["status"][:r].tolist(), lm_iterations=d["lm_iterations"][:r].tolist(),
                                  solves=d["n_solves"][:r].tolist(), cg_iterations=d["cg_iterations"][:r].tolist(), cg_capped=d["cg_capped"][:r].tolist(),
                                  inliers=d["inliers"][:r].tolist(), cost_initial=d["cost_initial"][:r].tolist(), cost_final=d["cost_final"][:r].tolist(),
                                  launches=d["launches"], launches_estimate=estimate(r, 5, d["n_solves"][:r], d["cg_iterations"][:r]),
                                  bit_identical=bool(same), one_core_ms=one_core * 1e3),
                   global_ba=dict(stats(g_ts), status=gres.status, lm_iterations=gres.lm_iterations, solves=gres.n_solves,
                                  cg_iterations=gres.cg_iterations_total, cg_capped=gres.cg_capped, cost_initial=gres.cost_initial,
                                  cost_final=gres.cost_final, launches_estimate=estimate(1, 4, [gres.n_solves], [gres.cg_iterations_total])))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/sba_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               params=dict(rounds=prm.rounds, robust_rounds=prm.robust_rounds, iterations=list(prm.iterations), max_trials=prm.max_trials,
                           cg_max_iterations=prm.cg_max_iterations, cg_batch=prm.cg_batch, cg_tol=prm.cg_tol, min_rel_decrease=prm.min_rel_decrease,
                           baseline=prm.baseline, chi2_mono=prm.chi2_mono, chi2_stereo=prm.chi2_stereo, global_ba_iterations=GBA_ITERATIONS,
                           global_ba_huber=5.991),
               scene=dict(points_per_pose=POINTS_PER_POSE, observations_per_point=OBS_PER_POINT, levels=4, noise="0.5 x 2^level", stereo="half",
                          outliers=0.1), warmup=WARMUP, timed=TIMED, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
