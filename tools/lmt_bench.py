#!/usr/bin/env python3
"""Call times of ygz_hip_map_point_attributes (csrc/mpa.hip) and ygz_hip_stereo_local_map_indexed (csrc/slm_index.hip in front of csrc/slm.hip)
at the map of tools/lms_bench.py: 200 keyframes, 20000 points of 1 + Poisson(4) observations.  The points are random pixels of a 640 x 480
camera un-projected at 2 .. 10 m, the keyframe centres lie within half a metre of the origin, the descriptors are random; eight resident
frames (detected keypoints of a texture, 60 % with a depth) serve every batch.  Batches of 1, 64 and 512 frame entries with DISTINCT lists of
3660 points each, identity entry poses, no prior.

Per batch: the indexed call and every kernel of it from the context's kernel probe (HIP events around its launch; 2 warm-up and 10 timed runs
per kernel); baseline A, the route without this call: ygz_hip_stereo_local_map_slots on the sets gathered by the lists on the host (the
gather itself is outside the clock), one call up to 64 frames, eight calls of 64 at 512 frames, summed; T_out and status compared on bits.
For the attributes: the call, its kernel, and baseline B, mr_attributes of tests/mpa_ref.c (gcc -O2) on one core.  The clock stands around
the Python binding with outputs=False and arrays already in the ABI's types.  Not timed: the object-graph gather of a host class.  3 warm-up
calls, then 20 timed; median / p10 / p90.  Usage (on the GPU box): tools/lmt_bench.py [out.json]; default profiles/lmt_bench.json."""
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
import mpa_ref as mr                          # noqa: E402  (test infrastructure: the one-core restatement)
import stereo_ref as sr                       # noqa: E402  (the texture)
from ygz_slam_amd import _lib                 # noqa: E402

K, N_POINTS, MEAN_OBS, LIST_LEN, SLOTS = 200, 20000, 5.0, 3660, 8
W, H, FX, CX, CY = 640, 480, 500.0, 320.0, 240.0
FRAMES = [1, 64, 512]
KERNELS = ["k_slm_index", "k_slm_gather", "k_strack_search", "k_slm_resolve", "k_pose_opt", "k_slm_scatter"]
WARMUP, TIMED = 3, 20


def stats(ts, scale=1e3):
    ts = np.asarray(ts) * scale
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def timed(call, warmup=WARMUP, n=TIMED):
    ts = []
    for k in range(warmup + n):
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if k >= warmup:
            ts.append(t1 - t0)
    return ts


def probe(ctx, kern, call, warmup=2, n=10):
    ms = []
    for k in range(warmup + n):
        ctx.probe_begin(kern, 16)
        call()
        t, launches = ctx.probe_end()
        assert launches >= 1, kern
        if k >= warmup:
            ms.append(t)
    return stats(ms, 1.0)


def r256(x):
    return (x + 255) // 256 * 256


def resident_frames(ctx, rng):
    """SLOTS resident frames: detected keypoints of a texture, 60 % with a depth; the keypoint counts"""
    tex = sr.texture(W + 8 * SLOTS, H, 5)
    for s in range(SLOTS):
        ctx.upload_gray(s, np.ascontiguousarray(tex[:, 8 * s:8 * s + W]))
    ctx.build_pyramid(0, SLOTS)
    ctx.detect(0, SLOTS)
    counts = ctx.get_keypoints_batch(0, SLOTS)["count"]
    for s in range(SLOTS):
        n = int(counts[s])
        ctx.set_keypoint_depths(s, rng.uniform(2, 10, n), (rng.uniform(size=n) < 0.6).astype(np.uint8))
    return counts


def make_map(rng):
    """the map (also tools/rmap_bench.py's): center, pw, off, kf, level as tests/mpa_ref.py names them, and per point the first observer
    (start) and the number of observers (n_obs), which are consecutive keyframes"""
    n_obs = np.clip(1 + rng.poisson(MEAN_OBS - 1.0, N_POINTS), 1, K).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32)
    start = rng.integers(0, K - n_obs + 1)
    kf = (np.repeat(start, n_obs) + np.arange(off[-1]) - np.repeat(off[:-1], n_obs)).astype(np.int32)
    level = rng.integers(0, 3, len(kf)).astype(np.int32)
    center = rng.uniform(-0.5, 0.5, (K, 3))
    z = rng.uniform(2, 10, N_POINTS)
    px = np.stack([rng.uniform(0, W, N_POINTS), rng.uniform(0, H, N_POINTS)], 1)
    pw = np.stack([(px[:, 0] - CX) / FX * z, (px[:, 1] - CY) / FX * z, z], 1)
    return dict(center=center, pw=pw, off=off, kf=kf, level=level, start=start, n_obs=n_obs)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lmt_bench.json")
    rng = np.random.default_rng(31)
    ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=SLOTS)
    counts = resident_frames(ctx, rng)
    m = make_map(rng)
    center, pw, off, kf, level = m["center"], m["pw"], m["off"], m["kf"], m["level"]
    att = ctx.map_point_attributes(center, pw, off, kf, level)
    ref = mr.attributes(m)
    mr.same(att, ref)
    a = mr.arrays(m)
    mpa_up = sum(r256(b) for b in (24 * K, 24 * N_POINTS, 4 * (N_POINTS + 1), 4 * len(kf), 4 * len(kf)))
    mpa_back = sum(r256(b) for b in (8 * N_POINTS, 24 * N_POINTS, 4 * N_POINTS))
    mpa_call = lambda: ctx.map_point_attributes(a["center"], a["pw"], a["off"], a["kf"], a["level"])      # noqa: E731
    attributes = dict(keyframes=K, points=N_POINTS, observations=int(len(kf)), bit_identical=True, call=stats(timed(mpa_call)),
                      kernel=probe(ctx, "k_mpa_attr", mpa_call), upload_bytes=int(mpa_up), copy_back_bytes=int(mpa_back),
                      one_core=stats(timed(lambda: mr.attributes(m), 1, 5)))
    attributes["speedup"] = attributes["one_core"]["median_ms"] / attributes["call"]["median_ms"]
    print(json.dumps(attributes), flush=True)
    pts = dict(pw=pw, pt_desc=rng.integers(0, 256, (N_POINTS, 32)).astype(np.uint8), pt_dmax=att["dmax"], pt_normal=att["normal"])
    I = np.array([0, 0, 0, 1.0, 0, 0, 0])
    rows = []
    for F in FRAMES:
        lp = np.stack([rng.permutation(N_POINTS)[:LIST_LEN] for _ in range(F)]).astype(np.int32)
        ll = np.full(F, LIST_LEN, np.int32)
        slots, li, T = (np.arange(F) % SLOTS).astype(np.int32), np.arange(F, dtype=np.int32), np.tile(I, (F, 1))
        indexed = lambda: ctx.stereo_local_map_indexed(pts, lp, ll, slots, li, T, outputs=False)           # noqa: E731
        sets = [{k: np.ascontiguousarray(v[lp[f]]) for k, v in pts.items()} for f in range(F)]

        def by_value():
            res = []
            for b in range(0, F, 64):
                e = min(b + 64, F)
                res.append(ctx.stereo_local_map_slots(sets[b:e], slots[b:e], np.arange(e - b, dtype=np.int32), T[b:e], outputs=False))
            return res
        got, want = indexed(), by_value()
        same = all(np.array_equal(got[k].view(np.uint64 if k == "T_out" else np.int32),
                                  np.concatenate([w[k] for w in want]).view(np.uint64 if k == "T_out" else np.int32)) for k in ("T_out", "status"))
        kernels = {kern: probe(ctx, kern, indexed) for kern in KERNELS}
        call, base = stats(timed(indexed)), stats(timed(by_value))
        N = F * LIST_LEN
        row = dict(frames=F, lists=F, list_length=LIST_LEN, pairs=N, keypoints_mean=float(counts.mean()), bit_identical=bool(same),
                   optimised=int((got["status"] == 0).sum()),
                   indexed=dict(call=call, kernels=kernels, kernels_ms=sum(v["median_ms"] for v in kernels.values()),
                                map_and_list_upload_bytes=int(r256(24 * N_POINTS) * 2 + r256(32 * N_POINTS) + r256(8 * N_POINTS) + r256(4 * N))),
                   by_value=dict(calls=(F + 63) // 64, total=base, set_upload_bytes=int(88 * N)),
                   speedup=base["median_ms"] / call["median_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/lmt_bench.py", date=datetime.date.today().isoformat(), device=_lib_device(), host=platform.processor() or platform.machine(),
               warmup=WARMUP, timed=TIMED, attributes=attributes, rows=rows,
               note="call: host clock around the Python binding (outputs=False: T_out and status alone come back); kernels: HIP events around the "
                    "launch of each kernel, one kernel per run; by_value: ygz_hip_stereo_local_map_slots on host-gathered sets, the gather outside "
                    "the clock, eight calls of 64 summed at 512 frames; one_core: mr_attributes of tests/mpa_ref.c (gcc -O2); not timed: the "
                    "object-graph gather of a host class")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    assert all(r["bit_identical"] for r in rows)


def _lib_device():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


if __name__ == "__main__":
    main()
