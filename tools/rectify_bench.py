#!/usr/bin/env python3
"""Kernel time of k_rectify (stereo rectification, csrc/rectify.hip) on 512 resident 640 x 480 frames -- 256 pairs of the test rig of
tests/rect_ref.py, cameras alternating slot by slot -- in one ygz_hip_build_pyramid_rectified call, for BGR and for gray uploads; beside it, in
the same session, k_undistort on the same frames with the left lens alone (the lens-only remap: the number to compare with) and k_bgr2gray16
on the same BGR frames (the colour conversion moves the same 4 bytes per pixel, 3 read and 1 written: the yardstick of DESIGN.md section
18).  Times come from the context's kernel probe (HIP events around every launch of the named kernel): 5 warm-up runs, then 50 timed; median
(p10 - p90); every row is measured twice, the rows alternating.  Bytes are what the algorithm needs (source picture + level 0; the maps, 8 bytes
per pixel and camera, are counted apart).  Slots 0, 1 and 511 are compared with the restatement (tests/rect_ref.c) bit for bit.  Usage (on the
GPU box): tools/rectify_bench.py [out.json]; the default output is profiles/rectify_bench.json."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rect_ref as rr                         # noqa: E402  (test infrastructure: the restatement)
import undist_ref as ur                       # noqa: E402
from ygz_slam_amd import _lib                 # noqa: E402

W, H, SLOTS, DISTINCT = 640, 480, 512, 32
WARMUP, TIMED, PASSES = 5, 50, 2


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


def probe(ctx, kernel, call, before=None):
    ms = []
    for k in range(WARMUP + TIMED):
        if before is not None:
            before()
        ctx.probe_begin(kernel, 16)
        call()
        t, n = ctx.probe_end()
        assert n == 1, (kernel, n)
        if k >= WARMUP:
            ms.append(t)
    return ms


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rectify_bench.json")
    rng = np.random.default_rng(23)
    frames = {True: rng.integers(0, 256, (DISTINCT, H, W, 3), dtype=np.uint8), False: rng.integers(0, 256, (DISTINCT, H, W), dtype=np.uint8)}
    ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=SLOTS)
    p0, p1, baseline = rr.rig()
    maps = []
    for k, p in enumerate((p0, p1)):
        ctx.set_rectification(k, R=np.array(list(p.R)), **{n: getattr(p.lens, n) for n, _ in p.lens._fields_})
        maps.append(rr.build_map(W, H, p))
    same_maps = all(np.array_equal(a, b) for k in range(2) for a, b in zip(ctx.rectify_map(k), maps[k]))
    ctx.set_undistortion(**{n: getattr(p0.lens, n) for n, _ in p0.lens._fields_})
    cams = np.arange(SLOTS, dtype=np.uint8) % 2
    npix = W * H
    rows, same = {}, {}

    def upload(bgr):
        for s in range(0, SLOTS, DISTINCT):
            (ctx.upload_bgr_batch if bgr else ctx.upload_gray_batch)(s, frames[bgr])

    def rectified_ok(bgr):
        return all(np.array_equal(ctx.download_level(s, 0), ur.remap(frames[bgr][s % DISTINCT], *maps[s % 2], 0)) for s in (0, 1, SLOTS - 1))

    for bgr in (True, False):
        tag = "bgr" if bgr else "gray"
        upload(bgr)
        # a gray run overwrites level 0, its own source: the raw pictures go up again before every run, outside the probe
        again = None if bgr else (lambda: upload(False))
        nbytes = SLOTS * npix * (4 if bgr else 2)
        for rep in range(PASSES):
            t = probe(ctx, "k_rectify", lambda: ctx.build_pyramid_rectified(cams, from_bgr=bgr), again)
            rows["k_rectify_%s_pass%d" % (tag, rep)] = stats(t, nbytes)
            same["k_rectify_%s_pass%d" % (tag, rep)] = bool(rectified_ok(bgr))
            t = probe(ctx, "k_undistort", lambda: ctx.build_pyramid_undistorted(0, SLOTS, from_bgr=bgr), again)
            rows["k_undistort_%s_pass%d" % (tag, rep)] = stats(t, nbytes)
            if bgr:
                t = probe(ctx, "k_bgr2gray", lambda: ctx.build_pyramid(0, SLOTS, from_bgr=True))
                rows["k_bgr2gray16_pass%d" % rep] = stats(t, nbytes)
    ctx.close()
    doc = dict(tool="tools/rectify_bench.py", date=datetime.date.today().isoformat(), device=device_name(), width=W, height=H, slots=SLOTS,
               pairs=SLOTS // 2, baseline=baseline, map_bytes_per_camera=W * H * 8, maps_bit_identical=bool(same_maps), warmup=WARMUP, timed=TIMED,
               rows=rows, bit_identical=same)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
