#!/usr/bin/env python3
"""Kernel time of k_undistort (lens undistortion, csrc/undistort.hip) on 512 resident 640 x 480 frames, for BGR and for gray uploads, beside
k_bgr2gray16 on the same BGR frames in the same session: the colour conversion moves the same 4 bytes per pixel (3 read, 1 written) and is the
yardstick.  The TUM fr1 coefficients on the context's default camera.  Times come from the context's kernel probe (HIP events around every
launch of the named kernel): one ygz_hip_build_pyramid_undistorted / ygz_hip_build_pyramid over all 512 slots per run, 5 warm-up runs, then 50
timed; median (p10 - p90).  Bytes are what the algorithm needs (source picture + level 0; the map, 8 bytes per pixel shared by every slot,
is counted apart).  Slots 0 and 511 are compared with the restatement (tests/undist_ref.c) bit for bit.  Usage (on the GPU box):
tools/undistort_bench.py [out.json]; the default output is profiles/undistort_bench.json."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import undist_ref as ur                       # noqa: E402  (test infrastructure: the restatement)
from ygz_slam_amd import _lib                 # noqa: E402

W, H, SLOTS, DISTINCT = 640, 480, 512, 32
WARMUP, TIMED = 5, 50


def stats(ms, bytes_moved):
    ms = np.asarray(ms)
    med = float(np.median(ms))
    return dict(median_ms=med, p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), runs=len(ms),
                bytes=int(bytes_moved), tb_per_s=bytes_moved / (med * 1e-3) / 1e12)


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def probe(ctx, kernel, call):
    ms = []
    for k in range(WARMUP + TIMED):
        ctx.probe_begin(kernel, 16)
        call()
        t, n = ctx.probe_end()
        assert n == 1, (kernel, n)
        if k >= WARMUP:
            ms.append(t)
    return ms


def measure(ctx, frames_bgr, frames_gray, ref_map, border=0):
    """dict of the three rows on a context whose map is set"""
    npix = W * H
    for s in range(0, SLOTS, DISTINCT):
        ctx.upload_bgr_batch(s, frames_bgr)
    t_conv = probe(ctx, "k_bgr2gray", lambda: ctx.build_pyramid(0, SLOTS, from_bgr=True))
    t_bgr = probe(ctx, "k_undistort", lambda: ctx.build_pyramid_undistorted(0, SLOTS, from_bgr=True))
    same_bgr = all(np.array_equal(ctx.download_level(s, 0), ur.remap(frames_bgr[s % DISTINCT], *ref_map, border)) for s in (0, SLOTS - 1))

    def gray_run():
        ctx.build_pyramid_undistorted(0, SLOTS, from_bgr=False)
    t_gray = []
    for k in range(WARMUP + TIMED):               # level 0 is overwritten by every run: the raw pictures go up again, outside the probe
        for s in range(0, SLOTS, DISTINCT):
            ctx.upload_gray_batch(s, frames_gray)
        ctx.probe_begin("k_undistort", 16)
        gray_run()
        t, n = ctx.probe_end()
        assert n == 1
        if k >= WARMUP:
            t_gray.append(t)
    same_gray = all(np.array_equal(ctx.download_level(s, 0), ur.remap(frames_gray[s % DISTINCT], *ref_map, border)) for s in (0, SLOTS - 1))
    return dict(k_bgr2gray16=stats(t_conv, SLOTS * npix * 4),
                k_undistort_bgr=dict(stats(t_bgr, SLOTS * npix * 4), bit_identical=bool(same_bgr)),
                k_undistort_gray=dict(stats(t_gray, SLOTS * npix * 2), bit_identical=bool(same_gray)))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "undistort_bench.json")
    rng = np.random.default_rng(23)
    frames_bgr = rng.integers(0, 256, (DISTINCT, H, W, 3), dtype=np.uint8)
    frames_gray = rng.integers(0, 256, (DISTINCT, H, W), dtype=np.uint8)
    ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=SLOTS)
    p = ctx.set_undistortion(**ur.TUM_FR1)
    ref = ur.params(ur.DEFAULT_CAMERA, **ur.TUM_FR1)
    ref_map = ur.build_map(W, H, ref, ur.DEFAULT_CAMERA)
    qx, qy = ctx.undistort_map()
    rows = measure(ctx, frames_bgr, frames_gray, ref_map)
    ctx.close()
    rows["ratio_bgr_to_bgr2gray16"] = rows["k_undistort_bgr"]["median_ms"] / rows["k_bgr2gray16"]["median_ms"]
    doc = dict(tool="tools/undistort_bench.py", date=datetime.date.today().isoformat(), device=device_name(), width=W, height=H, slots=SLOTS,
               coefficients={k: getattr(p, k) for k in ("k1", "k2", "p1", "p2", "k3")}, map_bytes=W * H * 8,
               map_bit_identical=bool(np.array_equal(qx, ref_map[0]) and np.array_equal(qy, ref_map[1])), warmup=WARMUP, timed=TIMED, rows=rows)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
