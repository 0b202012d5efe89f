#!/usr/bin/env python3
"""Kernel, device and call time of the stereo odometry on resident slots (csrc/svo.hip) at 1, 64 and 512 pairs of a 640 x 480 sequence with
1000 and with 3072 keypoints per frame (3072 = ygz_hip_max_keypoints), 60 % of them with a depth.  The frames are windows of one texture that
move by 3 pixels per frame, back and forth, every frame in a slot of its own (pair p = slots p, p + 1); the keypoints move with the pictures.

Per shape: every kernel of the call from the context's kernel probe (HIP events around its launches, the two launches of the search and of the
resolve summed; 3 warm-up and 20 timed runs per kernel), the device span from HIP events around upload, launches and copy back, and the call
from the host clock around the whole entry point (5 warm-up, 50 timed; median, p10 - p90).  Beside it the route the library offered before
for the same pairs: ygz_hip_get_keypoints_batch for all slots, the un-projection and the right columns in numpy, ygz_hip_stereo_track_search
in calls of 8 pairs (every pair has a point set of its own and a call takes YGZ_STRACK_MAX_SETS = 8 sets), the pairs below min_matches once
more with twice the window, the edge lists in numpy, one ygz_hip_optimize_pose_stereo for all pairs (5 warm-up and 50 timed runs at 1 and 64
pairs, 2 and 10 at 512).  The depths are taken as already on the host there (ygz_hip_stereo_depths_slots returns them).  T_rel, status and
the matches of the two routes are compared bit for bit in the same run.  No time is fixed in advance: the file records what was measured and
on which device.  Usage (on the GPU box): tools/svo_bench.py [out.json]; the default output is profiles/svo_bench.json."""
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stereo_ref as sr                       # noqa: E402  (test infrastructure: the texture)
import svo_ref as sv                          # noqa: E402  (the three formulas of the composition)
from ygz_slam_amd import _lib                 # noqa: E402

WARMUP, TIMED = 5, 50
W, H, SHIFT, Z, PERIOD = 640, 480, 3, 4.0, 7
PAIRS = [1, 64, 512]
KEYPOINTS = [1000, 3072]
KERNELS = ["k_svo_gather", "k_strack_search", "k_svo_resolve", "k_pose_opt", "k_svo_scatter"]


def stats(ms):
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), runs=len(ms))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def timed(call, warmup, runs):
    ms = []
    for k in range(warmup + runs):
        t0 = time.perf_counter()
        call()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def fill(ctx, n_frames, n_kp, seed):
    """frame k = the texture's window at offset tri(k) * SHIFT, its keypoints the scene's points at that offset; returns the host depths"""
    rng = np.random.default_rng(seed)
    src = sr.texture(W + SHIFT * PERIOD, H, seed)
    x0, y0 = rng.uniform(16 + SHIFT * PERIOD, W - 16, n_kp), rng.uniform(16, H - 16, n_kp)
    level, angle = rng.integers(0, 3, n_kp).astype(np.int32), rng.uniform(0, 360, n_kp).astype(np.float32)
    depth = np.full((n_frames, ctx.cells), -1.0)
    has = np.zeros((n_frames, ctx.cells), np.uint8)
    for k in range(n_frames):
        o = k % (2 * PERIOD)
        o = (o if o < PERIOD else 2 * PERIOD - o) * SHIFT
        ctx.upload_gray(k, np.ascontiguousarray(src[:, o:o + W]))
        ctx.build_pyramid(k, 1)
        ctx.describe_given_angle(k, np.stack([x0 - o, y0], 1), level, angle)
        has[k, :n_kp] = rng.uniform(size=n_kp) < 0.6
        depth[k, :n_kp] = np.where(has[k, :n_kp], Z, -1.0)
    ctx.set_keypoint_depths_batch(0, depth, has)
    return depth, has


def old_route(ctx, n_pairs, depth, has, K, p):
    """what a caller had to do before: fetch, search in calls of 8 pairs, retry, build edges, optimise"""
    kp = ctx.get_keypoints_batch(0, n_pairs + 1)
    cnt = kp["count"]
    fr = []
    for s in range(n_pairs + 1):
        m = int(cnt[s])
        hd = sv.has_depth(depth[s, :m], has[s, :m])
        pw, skip = sv.unproject(kp["px"][s, :m], depth[s, :m], hd, K)
        fr.append(dict(pw=pw, skip=skip, ur=sv.right_columns(kp["px"][s, :m], depth[s, :m], hd, p.baseline, K), px=kp["px"][s, :m],
                       level=kp["level"][s, :m], desc=kp["desc"][s, :m], angle=kp["angle"][s, :m].astype(np.float64)))
    T = np.array([0, 0, 0, 1.0, 0, 0, 0])
    match = [None] * n_pairs

    def search(which, th):
        for b in range(0, len(which), _lib.STRACK_MAX_SETS):
            part = which[b:b + _lib.STRACK_MAX_SETS]
            sets = [dict(pw=fr[q]["pw"], pt_desc=fr[q]["desc"], pt_level=fr[q]["level"], pt_angle=fr[q]["angle"]) for q in part]
            pbs = [dict(T=T, th=th, mode=0, direction=0, kp_px=fr[q + 1]["px"], kp_level=fr[q + 1]["level"], kp_desc=fr[q + 1]["desc"],
                        kp_ur=fr[q + 1]["ur"], kp_angle=fr[q + 1]["angle"], pt_skip=fr[q]["skip"], set=i) for i, q in enumerate(part)]
            o = ctx.stereo_track_search(sets, pbs, K, baseline=p.baseline, th_dist=p.th_dist, check_orientation=p.check_orientation)
            for i, q in enumerate(part):
                match[q] = (o["match"][o["offsets"][i]:o["offsets"][i + 1]], int(o["counts"][i, 0]))
    search(list(range(n_pairs)), p.th)
    again = [q for q in range(n_pairs) if match[q][1] < p.min_matches]
    if again:
        search(again, 2.0 * p.th)
    off, X, obs, lvl, kind, status = [0], [], [], [], [], np.zeros(n_pairs, np.int32)
    for q in range(n_pairs):
        status[q] = 1 if match[q][1] < p.min_matches else 0
        m = match[q][0] if status[q] == 0 else np.full(len(match[q][0]), -1)
        _, x, ob, lv, kd = sv.edges(m, fr[q]["pw"], fr[q + 1]["px"], fr[q + 1]["ur"], fr[q + 1]["level"])
        X.append(x); obs.append(ob); lvl.append(lv); kind.append(kd); off.append(off[-1] + len(lv))
    pose = ctx.default_pose_opt_params(baseline=p.baseline)
    r = ctx.optimize_pose_stereo(off, np.concatenate(X), np.concatenate(obs), np.concatenate(lvl), np.concatenate(kind),
                                 np.tile(T, (n_pairs, 1)), params=pose, outputs=False)
    return r["pose"], status, [m[0] for m in match]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "svo_bench.json")
    rows, same = {}, {}
    for n_kp in KEYPOINTS:
        ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=max(PAIRS) + 1)
        assert ctx.cells == 3072
        K = tuple(float(np.float32(getattr(ctx.params, k))) for k in ("fx", "fy", "cx", "cy"))
        depth, has = fill(ctx, max(PAIRS) + 1, n_kp, 40 + n_kp)
        p = ctx.default_svo_params()
        for n_pairs in PAIRS:
            key = "%dx_kp%d" % (n_pairs, n_kp)
            last, cur = np.arange(n_pairs), np.arange(1, n_pairs + 1)
            call = lambda: ctx.stereo_odometry_slots(last, cur, params=p, outputs=False)   # noqa: E731
            got = ctx.stereo_odometry_slots(last, cur, params=p)
            pose, status, match = old_route(ctx, n_pairs, depth, has, K, p)
            same[key] = bool(pose.tobytes() == got["T_rel"].tobytes() and np.array_equal(status, got["status"]) and
                             all(np.array_equal(m, got["match"][q, :len(m)]) for q, m in enumerate(match)))
            row = dict(pairs=n_pairs, keypoints=n_kp, matches=int(got["counts"][:, 3].sum()), retried=int(got["counts"][:, 7].sum()),
                       failed=int(got["status"].sum()), inliers=int(got["inliers"].sum()), kernels={})
            for kern in KERNELS:
                ms = []
                for k in range(3 + 20):
                    ctx.probe_begin(kern, 16)
                    call()
                    t, n = ctx.probe_end()
                    assert n == (2 if kern in ("k_strack_search", "k_svo_resolve") else 1), (kern, n)
                    if k >= 3:
                        ms.append(t)
                row["kernels"][kern] = stats(ms)
            span = []
            for k in range(WARMUP + TIMED):
                ctx.timer_begin()
                call()
                t = ctx.timer_end()
                if k >= WARMUP:
                    span.append(t)
            row["device_span"] = stats(span)
            row["call"] = timed(call, WARMUP, TIMED)
            row["call_all_outputs"] = timed(lambda: ctx.stereo_odometry_slots(last, cur, params=p), 2, 10)
            row["old_route"] = timed(lambda: old_route(ctx, n_pairs, depth, has, K, p), *((WARMUP, TIMED) if n_pairs <= 64 else (2, 10)))
            row["pairs_per_second"] = n_pairs / (row["call"]["median_ms"] * 1e-3)
            row["old_route_pairs_per_second"] = n_pairs / (row["old_route"]["median_ms"] * 1e-3)
            rows[key] = row
            print(key, json.dumps(row), "same" if same[key] else "DIFFERENT", flush=True)
        ctx.close()
    doc = dict(tool="tools/svo_bench.py", date=datetime.date.today().isoformat(), device=device_name(), warmup=WARMUP, timed=TIMED, rows=rows,
               bit_identical_to_old_route=same,
               note="kernels: HIP events around the launches of one kernel per run (search and resolve: both launches summed); device_span: HIP "
                    "events around upload, launches and copy back; call: the Python binding's wall clock around the entry point with only T_rel "
                    "and status asked for; call_all_outputs: every output asked for; old_route: get_keypoints_batch, numpy, "
                    "ygz_hip_stereo_track_search in calls of 8 pairs, the retry, numpy edges, ygz_hip_optimize_pose_stereo")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
