#!/usr/bin/env python3
"""Times of the stereo stage (csrc/stereo.hip) on 256 rectified 640 x 480 pairs resident in 512 slots, with detector keypoints and a shift of
20 pixels (16 distinct pairs, repeated), beside ygz_hip_detect over the same 512 slots in the same run: detect is what a stereo front end pays
per pair anyway, so it is the figure to compare against.  One ygz_hip_stereo_depths_slots call over all pairs per run: the whole call by HIP
events on the context's stream (upload of the pair table, two kernels, copy back), k_stereo_match and k_stereo_median by the context's kernel
probe.  k_stereo_match is also timed with th_dist = 0, where every keypoint stops after the descriptor search: that is the share of the
candidate filter and the Hamming distances (steps 1-3).  5 warm-up runs, then 30 timed; median (p10 - p90).  Pair 0 and pair 255 are compared
with the restatement (tests/stereo_ref.c) bit for bit.  Usage (on the GPU box): tools/stereo_bench.py [out.json]; the default output is
profiles/stereo_bench.json."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stereo_ref as sr                       # noqa: E402  (test infrastructure: the restatement and the textures)
from ygz_slam_amd import _lib                 # noqa: E402

W, H, PAIRS, DISTINCT, SHIFT = 640, 480, 256, 16, 20
WARMUP, TIMED = 5, 30


def stats(ms):
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), runs=len(ms))


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


def events(ctx, call):
    ms = []
    for k in range(WARMUP + TIMED):
        ctx.timer_begin()
        call()
        t = ctx.timer_end()
        if k >= WARMUP:
            ms.append(t)
    return ms


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "stereo_bench.json")
    pics = np.ascontiguousarray(np.stack([im for q in range(DISTINCT) for im in sr.shifted_pair(W, H, SHIFT, 100 + q)]))      # left, right, left, ...
    ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=2 * PAIRS)
    for s in range(0, 2 * PAIRS, 2 * DISTINCT):
        ctx.upload_gray_batch(s, pics)
    ctx.build_pyramid(0, 2 * PAIRS)
    t_detect = events(ctx, lambda: ctx.detect(0, 2 * PAIRS))
    left, right = np.arange(0, 2 * PAIRS, 2, dtype=np.int32), np.arange(1, 2 * PAIRS, 2, dtype=np.int32)
    p = ctx.default_stereo_params()
    p0 = ctx.default_stereo_params(th_dist=0)
    t_call = events(ctx, lambda: ctx.stereo_depths_slots(left, right, p))
    t_match = probe(ctx, "k_stereo_match", lambda: ctx.stereo_depths_slots(left, right, p))
    t_median = probe(ctx, "k_stereo_median", lambda: ctx.stereo_depths_slots(left, right, p))
    t_search = probe(ctx, "k_stereo_match", lambda: ctx.stereo_depths_slots(left, right, p0))
    got = ctx.stereo_depths_slots(left, right, p)
    counts = ctx.get_keypoint_counts(0, 2 * PAIRS)
    same = True
    for q in (0, PAIRS - 1):
        a, b = int(left[q]), int(right[q])
        ka, kb = ctx.get_keypoints(a), ctx.get_keypoints(b)
        lv = [[ctx.download_level(s, l) for l in range(3)] for s in (a, b)]
        want = sr.match(lv[0], lv[1], sr.keypoints(ka["px"], ka["level"], ka["desc"]), sr.keypoints(kb["px"], kb["level"], kb["desc"]), sr.params())
        n = len(ka["level"])
        same = same and all(np.array_equal(got[k][q, :n], want[k]) for k in ("right_idx", "u_right", "depth", "sad", "status"))
        same = same and bool(np.array_equal(got["counts"][q], want["counts"]))
    ctx.close()
    rows = dict(detect_512_slots=stats(t_detect), stereo_depths_slots_call=stats(t_call), k_stereo_match=stats(t_match),
                k_stereo_median=stats(t_median), k_stereo_match_search_only=stats(t_search))
    rows["search_share_of_match"] = rows["k_stereo_match_search_only"]["median_ms"] / rows["k_stereo_match"]["median_ms"]
    rows["kernels_to_detect"] = (rows["k_stereo_match"]["median_ms"] + rows["k_stereo_median"]["median_ms"]) / rows["detect_512_slots"]["median_ms"]
    doc = dict(tool="tools/stereo_bench.py", date=datetime.date.today().isoformat(), device=device_name(), width=W, height=H, pairs=PAIRS,
               slots=2 * PAIRS, shift=SHIFT, keypoints_left=int(counts[0::2].sum()), keypoints_right=int(counts[1::2].sum()),
               status_counts=got["counts"].sum(axis=0).tolist(), bit_identical=bool(same), output_bytes=int(PAIRS * ctx.cells * 28 + PAIRS * 28),
               warmup=WARMUP, timed=TIMED, rows=rows)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
