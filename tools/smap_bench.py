#!/usr/bin/env python3
"""Kernel and call time of stereo map-point creation (csrc/smap.hip).  Workload: ten neighbours of 1000 matched pairs each in ONE
ygz_hip_stereo_create_map_points call -- the forward-motion scene of tests/smap_ref.py with true matches, the last third of every problem
turned into wrong matches (camera-2 pixels shifted by 3-30 px, depths off by 20 %), so that about a third of the pairs is triangulated, a third
un-projected and a third rejected; the measured shares are recorded -- and, separately, one keyframe of ygz_hip_max_keypoints features (640 x
480: 3072) through ygz_hip_stereo_keyframe_points.  Kernel times come from the context's kernel probe (HIP events around the launch), the call
times from the host clock around the whole entry point (upload, launch, copy back, wait): 5 warm-up runs, then 50 timed; median (p10 - p90).
Beside them the restatement's C functions (tests/smap_ref.c) alone on the same inputs on one host core.  Every output is compared with the
restatement bit for bit.  No time is fixed in advance: the file records what was measured and on which device.  Usage (on the GPU box): tools/smap_bench.py
[out.json]; the default output is profiles/smap_bench.json."""
import ctypes
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import smap_ref as sm                         # noqa: E402  (test infrastructure: the restatement)
from ygz_slam_amd import _lib                 # noqa: E402

NEIGHBOURS, PAIRS = 10, 1000
WARMUP, TIMED = 5, 50


def stats(ms):
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), runs=len(ms))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def problem(seed):
    pb = sm.scene("forward", PAIRS, seed, true_matches=True)
    rng = np.random.default_rng(1000 + seed)
    k = PAIRS - PAIRS // 3
    n = PAIRS - k
    r, a = rng.uniform(3.0, 30.0, n), rng.uniform(0, 2 * np.pi, n)
    pb["px2"][k:] += np.stack([r * np.cos(a), r * np.sin(a)], 1)
    pb["depth1"][k:] *= np.where(rng.random(n) < 0.5, 1.2, 0.8)
    pb["depth2"][k:] *= np.where(rng.random(n) < 0.5, 1.2, 0.8)
    return pb


def measure(ctx, kernel, call):
    kernel_ms, call_ms = [], []
    for k in range(WARMUP + TIMED):
        ctx.probe_begin(kernel, 16)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        t, n = ctx.probe_end()
        assert n == 1, (kernel, n)
        if k >= WARMUP:
            kernel_ms.append(t)
            call_ms.append((t1 - t0) * 1e3)
    return stats(kernel_ms), stats(call_ms)


def host(call):
    ms = []
    for k in range(WARMUP + TIMED):
        t0 = time.perf_counter()
        call()
        if k >= WARMUP:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "smap_bench.json")
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2, intrinsics=sm.K4)
    pbs = [problem(40 + q) for q in range(NEIGHBOURS)]
    p = ctx.default_smap_params()
    got = ctx.stereo_create_map_points(pbs, sm.K4, params=p)
    ref = [sm.create(pb) for pb in pbs]
    code, method, pos = np.concatenate([r[0] for r in ref]), np.concatenate([r[1] for r in ref]), np.concatenate([r[2] for r in ref])
    same_pairs = bool(np.array_equal(got["code"], code) and np.array_equal(got["method"], method) and got["pos_world"].tobytes() == pos.tobytes())
    N = len(code)
    shares = dict(triangulated=float(((code == 0) & (method == 1)).sum() / N), unprojected=float(((code == 0) & (method >= 2)).sum() / N),
                  rejected=float((code != 0).sum() / N), entered_the_jacobi=float((method == 1).sum() / N))
    rows = {}
    rows["k_smap_pairs"], rows["stereo_create_map_points_call"] = measure(ctx, "k_smap_pairs", lambda: ctx.stereo_create_map_points(pbs, sm.K4, params=p))
    # the restatement's C functions alone: structs, parameters and output arrays are made once, outside the clock
    L, dbl, i32, u8 = sm.lib(), ctypes.c_double, ctypes.c_int32, ctypes.c_uint8
    rp, k4 = sm.default_params(), np.ascontiguousarray(sm.K4, np.float64)
    norm = [sm.normalise(pb) for pb in pbs]
    calls = [(ctypes.byref(sm.c_problem(pb)), sm._p(np.zeros(pb["n"], np.int32), i32), sm._p(np.zeros(pb["n"], np.int32), i32),
              sm._p(np.zeros((pb["n"], 3)), dbl)) for pb in norm]
    rows["restatement_pairs_one_core"] = host(lambda: [L.sm_create(s_, sm._p(k4, dbl), ctypes.byref(rp), c_, m_, x_) for s_, c_, m_, x_ in calls])

    n = ctx.cells
    T, px, depth, has = sm.keyframe_scene(n, n - n // 10, n // 3, 9, ties=True)
    gk = ctx.stereo_keyframe_points(T, px, depth, has, sm.K4, params=p)
    rk = sm.keyframe_points(T, px, depth, has, sm.K4)
    same_kf = bool(np.array_equal(gk["rank"], rk["rank"]) and np.array_equal(gk["selected"], rk["selected"]) and
                   gk["pos_world"].tobytes() == rk["pos_world"].tobytes() and (gk["n_depth"], gk["n_close"]) == (rk["n_depth"], rk["n_close"]))
    rows["k_smap_keyframe"], rows["stereo_keyframe_points_call"] = measure(ctx, "k_smap_keyframe",
                                                                          lambda: ctx.stereo_keyframe_points(T, px, depth, has, sm.K4, params=p))
    Tc, pxc, dc, hc = [np.ascontiguousarray(a, t) for a, t in ((T, np.float64), (px, np.float64), (depth, np.float64), (has, np.uint8))]
    o_rank, o_sel, o_pos, o_nd, o_nc = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 3)), ctypes.c_int32(0), ctypes.c_int32(0)
    rows["restatement_keyframe_one_core"] = host(lambda: L.sm_keyframe_points(sm._p(Tc, dbl), sm._p(pxc, dbl), sm._p(dc, dbl), sm._p(hc, u8), n,
                                                                              sm._p(k4, dbl), ctypes.byref(rp), sm._p(o_rank, i32), sm._p(o_sel, u8),
                                                                              sm._p(o_pos, dbl), ctypes.byref(o_nd), ctypes.byref(o_nc)))
    ctx.close()
    doc = dict(tool="tools/smap_bench.py", date=datetime.date.today().isoformat(), device=device_name(), neighbours=NEIGHBOURS, pairs_per_neighbour=PAIRS,
               pair_shares=shares, keyframe_features=int(n), keyframe_n_depth=int(rk["n_depth"]), keyframe_n_close=int(rk["n_close"]),
               keyframe_selected=int(rk["selected"].sum()), warmup=WARMUP, timed=TIMED, rows=rows,
               bit_identical=dict(pairs=same_pairs, keyframe=same_kf),
               note="call rows: the Python binding's wall clock around the entry point, array packing of the binding included; restatement rows: the C functions alone, "
                    "structs and output arrays made outside the clock")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
