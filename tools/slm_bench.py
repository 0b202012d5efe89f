#!/usr/bin/env python3
"""Kernel, device and call time of the stereo local-map tracking on resident slots (csrc/slm.hip) at 1, 64 and 512 frames of a 640 x 480
sequence with 1000 and with 3072 keypoints per frame (3072 = ygz_hip_max_keypoints), 60 % of them with a depth, against a shared local map of
2000 and of 8000 points; half of every frame's keypoints already hold their point (prior).  The frames are windows of one texture that move by
3 pixels per frame, back and forth, every frame in a slot of its own; the keypoints move with the pictures.  The map's first points are the
scene's points under the keypoints (the keypoint's descriptor with up to 20 flipped bits), the rest lie anywhere in front of the camera.

Per shape: every kernel of the call from the context's kernel probe (HIP events around its launch; 3 warm-up and 20 timed runs per kernel),
the device span from HIP events around upload, launches and copy back, and the call from the host clock around the whole entry point (5
warm-up, 50 timed; median, p10 - p90), asking for T_out and status only and asking for every output.  Beside it the route the library offered
before for the same frames: ygz_hip_get_keypoints_batch for all slots, right columns, taken and skip flags in numpy,
ygz_hip_stereo_track_search in calls of at most 64 problems (and at most YGZ_STRACK_MAX_PAIRS pairs), the edge lists in numpy, one
ygz_hip_optimize_pose_stereo for all frames (5 warm-up and 50 timed runs at 1 and 64 frames, 2 and 10 at 512).  The depths are taken as
already on the host there.  T_out, status and the point behind every keypoint of the two routes are compared bit for bit in the same run.
No time is fixed in advance: the file records what was measured and on which device.  Usage (on the GPU box): tools/slm_bench.py [out.json];
the default output is profiles/slm_bench.json."""
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import proj_ref                               # noqa: E402  (test infrastructure: flip_bits)
import slm_ref as sl                          # noqa: E402  (the formulas of the composition)
import stereo_ref as sr                       # noqa: E402  (the texture)
from ygz_slam_amd import _lib                 # noqa: E402

WARMUP, TIMED = 5, 50
W, H, SHIFT, Z, PERIOD = 640, 480, 3, 4.0, 7
FRAMES = [1, 64, 512]
KEYPOINTS = [1000, 3072]
POINTS = [2000, 8000]
KERNELS = ["k_slm_gather", "k_strack_search", "k_slm_resolve", "k_pose_opt", "k_slm_scatter"]


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


def offset(k):
    o = k % (2 * PERIOD)
    return (o if o < PERIOD else 2 * PERIOD - o) * SHIFT


def fill(ctx, n_frames, n_kp, seed):
    """frame k = the texture's window at offset(k), its keypoints the scene's points at that offset; (depth, has, the scene's pixels at offset 0,
    level)"""
    rng = np.random.default_rng(seed)
    src = sr.texture(W + SHIFT * PERIOD, H, seed)
    x0, y0 = rng.uniform(16 + SHIFT * PERIOD, W - 16, n_kp), rng.uniform(16, H - 16, n_kp)
    level, angle = rng.integers(0, 3, n_kp).astype(np.int32), rng.uniform(0, 360, n_kp).astype(np.float32)
    depth = np.full((n_frames, ctx.cells), -1.0)
    has = np.zeros((n_frames, ctx.cells), np.uint8)
    for k in range(n_frames):
        o = offset(k)
        ctx.upload_gray(k, np.ascontiguousarray(src[:, o:o + W]))
        ctx.build_pyramid(k, 1)
        ctx.describe_given_angle(k, np.stack([x0 - o, y0], 1), level, angle)
        has[k, :n_kp] = rng.uniform(size=n_kp) < 0.6
        depth[k, :n_kp] = np.where(has[k, :n_kp], Z, -1.0)
    ctx.set_keypoint_depths_batch(0, depth, has)
    return depth, has, np.stack([x0, y0], 1), level


def local_map(ctx, px, level, n_pt, K, seed):
    """n_pt points in the first camera's frame: point i < n_kp under keypoint i of slot 0, the others anywhere in the picture at 3 .. 6 m"""
    rng = np.random.default_rng(seed)
    kp = ctx.get_keypoints_batch(0, 1)
    m = min(n_pt, len(level))
    u = np.concatenate([px[:m], np.stack([rng.uniform(0, W, n_pt - m), rng.uniform(0, H, n_pt - m)], 1)])
    z = np.concatenate([np.full(m, Z), rng.uniform(3, 6, n_pt - m)])
    lv = np.concatenate([level[:m], rng.integers(0, 3, n_pt - m)])
    pw = np.stack([(u[:, 0] - K[2]) / K[0] * z, (u[:, 1] - K[3]) / K[1] * z, z], 1)
    d = np.linalg.norm(pw, axis=1)
    desc = np.concatenate([np.stack([proj_ref.flip_bits(rng, kp["desc"][0, i], int(rng.integers(0, 21))) for i in range(m)]),
                           rng.integers(0, 256, (n_pt - m, 32)).astype(np.uint8)])
    return dict(pw=pw, pt_desc=desc, pt_dmax=2.0 ** lv * 0.9 * d, pt_normal=pw / d[:, None])


def old_route(ctx, n_frames, depth, has, s, T, prior, K, p):
    """what a caller had to do before: fetch, flags, search in calls of at most 64 problems, edges, optimise"""
    kp = ctx.get_keypoints_batch(0, n_frames)
    cnt = kp["count"]
    n_pt = len(s["pt_dmax"])
    pbs, fr = [], []
    for f in range(n_frames):
        m = int(cnt[f])
        ur = sl.right_columns(kp["px"][f, :m], depth[f, :m], sl.has_depth(depth[f, :m], has[f, :m]), p.baseline, K)
        pr, taken, skip = sl.prior_flags(prior[f], m, n_pt)
        fr.append((pr, ur, m))
        pbs.append(dict(T=T[f], th=p.th, mode=1, direction=0, kp_px=kp["px"][f, :m], kp_level=kp["level"][f, :m], kp_desc=kp["desc"][f, :m],
                        kp_ur=ur, kp_taken=taken, pt_skip=skip, set=0))
    per_call = max(1, min(_lib.STRACK_MAX_PROBLEMS, _lib.STRACK_MAX_PAIRS // n_pt))
    match = []
    for b in range(0, n_frames, per_call):
        o = ctx.stereo_track_search([s], pbs[b:b + per_call], K, baseline=p.baseline, ratio=p.ratio, r_near=p.r_near, r_wide=p.r_wide,
                                    cos_near=p.cos_near, th_dist=p.th_dist)
        match += [o["match"][o["offsets"][i]:o["offsets"][i + 1]] for i in range(len(o["offsets"]) - 1)]
    off, X, obs, lvl, kind, status, points = [0], [], [], [], [], np.zeros(n_frames, np.int32), []
    for f in range(n_frames):
        pr, ur, m = fr[f]
        kpp = sl.keypoint_points(pr, match[f])
        j, x, ob, lv, kd = sl.edges(kpp, s["pw"], kp["px"][f, :m], ur, kp["level"][f, :m])
        status[f] = 1 if len(j) < p.min_edges else 0
        keep = slice(0, 0) if status[f] else slice(None)
        X.append(x[keep]); obs.append(ob[keep]); lvl.append(lv[keep]); kind.append(kd[keep]); off.append(off[-1] + len(lv[keep]))
        points.append(kpp)
    pose = ctx.default_pose_opt_params(baseline=p.baseline)
    r = ctx.optimize_pose_stereo(off, np.concatenate(X), np.concatenate(obs), np.concatenate(lvl), np.concatenate(kind), T[:n_frames],
                                 params=pose, outputs=False)
    return r["pose"], status, points


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "slm_bench.json")
    rows, same = {}, {}
    for n_kp in KEYPOINTS:
        ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=max(FRAMES))
        assert ctx.cells == 3072
        K = tuple(float(np.float32(getattr(ctx.params, k))) for k in ("fx", "fy", "cx", "cy"))
        depth, has, px, level = fill(ctx, max(FRAMES), n_kp, 40 + n_kp)
        p = ctx.default_slm_params()
        T_all = np.stack([[0, 0, 0, 1.0, -offset(k) * Z / K[0], 0, 0] for k in range(max(FRAMES))])
        for n_pt in POINTS:
            s = local_map(ctx, px, level, n_pt, K, 7 + n_pt)
            held = np.full(ctx.cells, -1, np.int32)
            j = np.arange(0, min(n_kp, n_pt), 2)
            held[j] = j                                                  # every second keypoint holds the point under it
            for n_frames in FRAMES:
                key = "%dx_kp%d_pt%d" % (n_frames, n_kp, n_pt)
                slots, st, T = np.arange(n_frames), np.zeros(n_frames, np.int32), T_all[:n_frames]
                prior = np.tile(held, (n_frames, 1))
                call = lambda: ctx.stereo_local_map_slots([s], slots, st, T, prior, params=p, outputs=False)   # noqa: E731
                got = ctx.stereo_local_map_slots([s], slots, st, T, prior, params=p)
                pose, status, points = old_route(ctx, n_frames, depth, has, s, T, prior, K, p)
                same[key] = bool(pose.tobytes() == got["T_out"].tobytes() and np.array_equal(status, got["status"]) and
                                 all(np.array_equal(q, got["kp_point"][f, :len(q)]) for f, q in enumerate(points)))
                c = got["counts"]
                row = dict(frames=n_frames, keypoints=n_kp, points=n_pt, prior_edges=int(c[:, 2].sum()), searched=int(c[:, 4].sum()),
                           overflowed=int(c[:, 5].sum()), new_matches=int(c[:, 6].sum()), edges=int(c[:, 7].sum()),
                           failed=int(got["status"].sum()), inliers=int(got["inliers"].sum()), kernels={})
                for kern in KERNELS:
                    ms = []
                    for k in range(3 + 20):
                        ctx.probe_begin(kern, 16)
                        call()
                        t, n = ctx.probe_end()
                        assert n == 1, (kern, n)
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
                row["call_all_outputs"] = timed(lambda: ctx.stereo_local_map_slots([s], slots, st, T, prior, params=p), 2, 10)
                row["old_route"] = timed(lambda: old_route(ctx, n_frames, depth, has, s, T, prior, K, p),
                                         *((WARMUP, TIMED) if n_frames <= 64 else (2, 10)))
                row["frames_per_second"] = n_frames / (row["call"]["median_ms"] * 1e-3)
                row["old_route_frames_per_second"] = n_frames / (row["old_route"]["median_ms"] * 1e-3)
                rows[key] = row
                print(key, json.dumps(row), "same" if same[key] else "DIFFERENT", flush=True)
        ctx.close()
    doc = dict(tool="tools/slm_bench.py", date=datetime.date.today().isoformat(), device=device_name(), warmup=WARMUP, timed=TIMED, rows=rows,
               bit_identical_to_old_route=same,
               note="kernels: HIP events around the launch of one kernel per run; device_span: HIP events around upload, launches and copy "
                    "back; call: the Python binding's wall clock around the entry point with only T_out and status asked for; "
                    "call_all_outputs: every output asked for; old_route: get_keypoints_batch, numpy, ygz_hip_stereo_track_search in calls of "
                    "at most 64 problems, numpy edges, ygz_hip_optimize_pose_stereo")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    assert all(same.values()), same


if __name__ == "__main__":
    main()
