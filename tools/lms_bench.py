#!/usr/bin/env python3
"""Call time of ygz_hip_local_map_select (local-map selection, csrc/lms.hip) beside its restatement on one host core (tests/lms_ref.c, gcc -O2)
on the same arrays, with a bit-identity flag per row.  One map -- 200 keyframes, 20000 points of 1 + Poisson(4) observations on a run of
consecutive keyframes, as covisible keyframes are, the features of a keyframe numbered in a random order, ten covisible neighbours per
keyframe, nearest index first -- and three batches on it: 1, 64 and 512 frames of 1000 entries each, 800 of them points seen from within
three keyframes of a random centre.  max_keyframes 80, max_points 8192 (512 frames of more do not fit YGZ_SLM_MAX_PAIRS).

Per shape: every kernel of the call from the context's kernel probe (HIP events around its launch; 3 warm-up and 20 timed runs per kernel);
the call from a host clock around the C ABI entry point, which ends in its one wait (the arrays are marshalled once, outside the clock), with
votes left on the device and with every output; a host-to-device copy of the bytes the call uploads and a device-to-host copy of the bytes it
brings back, each alone, from page-locked memory, under the same clock; `host_and_waits_ms` is what is left of the call: the checks, the
keyframe-major index, packing, unpacking and the gaps.  Restatement: the median of 3 runs.  5 warm-up calls, then 50 timed; median / p10 /
p90.  Usage (on the GPU box): tools/lms_bench.py [out.json]; the default output is profiles/lms_bench.json."""
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
import lms_ref as lr                          # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402

K, N_POINTS, MEAN_OBS, N_COV, ENTRIES, ON_FRAME, MAX_KF, MAX_PT = 200, 20000, 5.0, 10, 1000, 800, 80, 8192
FRAMES = [1, 64, 512]
KERNELS = ["k_lms_vote", "k_lms_points", "k_lms_place", "k_lms_prior"]
WARMUP, TIMED = 5, 50


def stats(ts, scale=1e3):
    ts = np.asarray(ts) * scale
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def the_map(rng):
    n = np.clip(1 + rng.poisson(MEAN_OBS - 1.0, N_POINTS), 1, K).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    start = rng.integers(0, K - n + 1)
    kf = (np.repeat(start, n) + np.arange(off[-1]) - np.repeat(off[:-1], n)).astype(np.int32)
    feat = np.zeros(len(kf), np.int32)
    for k in range(K):                        # a keyframe's observations get distinct feature indices in a random order, with gaps
        at = np.flatnonzero(kf == k)
        feat[at] = rng.permutation(2 * len(at))[:len(at)]
    cov = np.zeros((K, N_COV), np.int32)
    for k in range(K):
        near = sorted((c for c in range(K) if c != k), key=lambda c: (abs(c - k), c))
        cov[k] = near[:N_COV]
    return off, kf, feat, cov, start, n


def frames_on(rng, n_frames, start, n):
    fr_pt = np.full((n_frames, ENTRIES), -1, np.int32)
    for f in range(n_frames):
        c = int(rng.integers(0, K))
        near = np.flatnonzero((start <= c + 3) & (start + n - 1 >= c - 3))
        fr_pt[f, rng.permutation(ENTRIES)[:ON_FRAME]] = rng.choice(near, ON_FRAME, replace=len(near) < ON_FRAME)
    return np.arange(n_frames + 1, dtype=np.int32) * ENTRIES, fr_pt.reshape(-1)


def timed(call, warmup=WARMUP, n=TIMED):
    ts = []
    for k in range(warmup + n):
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        assert rc == 0, rc
        if k >= warmup:
            ts.append(t1 - t0)
    return ts


def r256(x):
    return (x + 255) // 256 * 256


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lms_bench.json")
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    lib = ctx.lib
    _lib.lms_argtypes(lib)
    lib.ygz_hip_pinned_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.ygz_hip_pinned_free.argtypes = [C.c_void_p]
    lib.ygz_hip_device_alloc.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t]
    lib.ygz_hip_device_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.ygz_hip_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    P = lambda a, t=ip: a.ctypes.data_as(t)                                          # noqa: E731
    rng = np.random.default_rng(29)
    off, kf, feat, cov, start, n_obs_of = the_map(rng)
    kf_bad = np.zeros(K, np.uint8)
    prm = _lib.LmsParams(MAX_KF, MAX_PT)
    ref_lib = lr.lib()
    rows = []
    for F in FRAMES:
        fr_off, fr_pt = frames_on(rng, F, start, n_obs_of)
        E, N = len(fr_pt), len(kf)
        o = {k: np.full(s, -7, np.int32) for k, s in dict(votes=F * K, ref=F, n_voters=F, n_local=F, local_kf=F * K, n_pt=F, n_cut=F, local_pt=F * MAX_PT,
                                                          fr_prior=E).items()}
        r = {k: np.full(len(v), -8, np.int32) for k, v in o.items()}

        def device(votes=True):
            outs = [P(o[k]) if votes or k != "votes" else None for k in lr.OUTPUTS]
            return lib.ygz_hip_local_map_select(ctx._ctx, K, P(kf_bad, bp), N_COV, P(cov), N_POINTS, P(off), P(kf), P(feat), None, F, P(fr_off),
                                                P(fr_pt), C.byref(prm), *outs)

        def host():
            q = lr.Params(MAX_KF, MAX_PT)
            return ref_lib.lr_select(K, P(kf_bad, bp), N_COV, P(cov), N_POINTS, P(off), P(kf), P(feat), None, F, P(fr_off), P(fr_pt), C.byref(q),
                                     *[P(r[k]) for k in lr.OUTPUTS])
        assert device() == 0 and host() == 0
        same = all(np.array_equal(o[k], r[k]) for k in lr.OUTPUTS)
        kernels = {}
        for kern in KERNELS:
            ms = []
            for k in range(3 + 20):
                ctx.probe_begin(kern, 4)
                assert device(False) == 0
                t, n = ctx.probe_end()
                assert n == 1, (kern, n)
                if k >= 3:
                    ms.append(t)
            kernels[kern] = stats(ms, 1.0)
        call = stats(timed(lambda: device(False)))
        call_all = stats(timed(lambda: device(True)))
        one_core = stats(timed(host, 0, 3))
        # the bytes of the packed block (each array at a multiple of 256), copied alone
        up = sum(r256(b) for b in (K, N_POINTS, 4 * K * N_COV, 4 * (N_POINTS + 1), 4 * N, 4 * (K + 1), 4 * N, 4 * (F + 1), 4 * E))
        back = sum(r256(b) for b in (4 * F,) * 5 + (4 * F * K, 4 * F * MAX_PT, 4 * E))
        hp, dp = C.c_void_p(), C.c_void_p()
        assert lib.ygz_hip_pinned_alloc(C.byref(hp), max(up, back)) == 0 and lib.ygz_hip_device_alloc(ctx._ctx, C.byref(dp), max(up, back)) == 0
        upload = stats(timed(lambda: lib.ygz_hip_copy(ctx._ctx, dp, hp, up, 0, 1)))
        copy_back = stats(timed(lambda: lib.ygz_hip_copy(ctx._ctx, hp, dp, back, 1, 1)))
        lib.ygz_hip_device_free(ctx._ctx, dp)
        lib.ygz_hip_pinned_free(hp)
        kernel_ms = sum(v["median_ms"] for v in kernels.values())
        row = dict(frames=F, entries_per_frame=ENTRIES, points_per_frame=ON_FRAME, keyframes=K, points=N_POINTS, observations=int(N), n_cov=N_COV,
                   max_keyframes=MAX_KF, max_points=MAX_PT, local_keyframes_mean=float(o["n_local"].mean()), voters_mean=float(o["n_voters"].mean()),
                   local_points_mean=float(o["n_pt"].mean()), cut_mean=float(o["n_cut"].mean()), bit_identical=bool(same),
                   device=dict(call=call, call_with_votes=call_all, kernels=kernels, kernels_ms=kernel_ms, upload_bytes=int(up), upload_alone=upload,
                               copy_back_bytes=int(back), copy_back_alone=copy_back,
                               host_and_waits_ms=call["median_ms"] - kernel_ms - upload["median_ms"] - copy_back["median_ms"]),
                   one_core=one_core, speedup=one_core["median_ms"] / call["median_ms"],
                   frames_per_second=dict(device=F / (call["median_ms"] * 1e-3), one_core=F / (one_core["median_ms"] * 1e-3)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/lms_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               warmup=WARMUP, timed=TIMED, rows=rows,
               note="call: host clock around ygz_hip_local_map_select with votes NULL (call_with_votes: every output); kernels: HIP events around "
                    "the one launch of each kernel, one kernel per run; upload_alone / copy_back_alone: one hipMemcpy of the call's byte counts "
                    "between page-locked and device memory, outside the call; host_and_waits_ms = call - kernels - upload_alone - copy_back_alone; "
                    "one_core: lr_select of tests/lms_ref.c (gcc -O2) on the same arrays, 3 runs")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    assert all(r["bit_identical"] for r in rows)


if __name__ == "__main__":
    main()
