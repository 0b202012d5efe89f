#!/usr/bin/env python3
"""Kernel, device and call time of the stereo reference-keyframe tracking on resident slots (csrc/srk.hip) at 1, 64 and 512 frames of a
640 x 480 sequence with 1000 and with 3072 keypoints per frame (3072 = ygz_hip_max_keypoints), 60 % of them with a depth.  The frames are
windows of one texture that move by 3 pixels per frame, back and forth, every frame in a slot of its own; the keypoints move with the
pictures.  One keyframe per 32 frames (at least one), each in a slot of its own with the picture of offset 0; 60 % of a keyframe's keypoints
carry the scene's point under them.  The vocabulary is synthetic (k = 10, L = 5) and levelsup is 3, so that the FeatureVector has the about
100 nodes an ORB vocabulary of six levels has at levelsup 4.

Per shape: every kernel of the call from the context's kernel probe (HIP events around its launches; 3 warm-up and 20 timed runs per
kernel), the device span from HIP events around upload, launches and copy back, and the call from the host clock around the whole entry point
(5 warm-up, 50 timed; median, p10 - p90), asking for T_out, status and prior only and asking for every output.  Beside it the route the
library offered before for the same frames: ygz_hip_get_keypoints_batch for all slots, ygz_hip_compute_bow, ygz_hip_search_by_bow_slots, the
claim in numpy, ygz_hip_bow_orientation_slots for the maxima and the removal in numpy, the right columns and the edge lists in numpy, one
ygz_hip_optimize_pose_stereo for all frames (5 warm-up and 50 timed runs at 1 and 64 frames, 2 and 10 at 512).  The depths are taken as already
on the host there.  T_out, status and kp_point of the two routes are compared bit for bit in the same run.  No time is fixed in advance: the
file records what was measured and on which device.  Usage (on the GPU box): tools/srk_bench.py [out.json]; the default output is
profiles/srk_bench.json."""
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fixtures                               # noqa: E402  (test infrastructure: the synthetic vocabulary)
import srk_ref as sk                          # noqa: E402  (the formulas of the composition)
import stereo_ref as sr                       # noqa: E402  (the texture)
from ygz_slam_amd import _lib                 # noqa: E402

WARMUP, TIMED = 5, 50
W, H, SHIFT, Z, PERIOD = 640, 480, 3, 4.0, 7
FRAMES = [1, 64, 512]
KEYPOINTS = [1000, 3072]
LEVELSUP = 3
KERNELS = {"k_srk_gather": 2, "k_bow_transform": 1, "k_bow_match": 1, "k_srk_resolve": 1, "k_pose_opt": 1, "k_srk_scatter": 1}    # launches per call


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


def fill(ctx, n_frames, n_kf, n_kp, seed):
    """frame k = the texture's window at offset(k), its keypoints the scene's points at that offset; the keyframes behind them, at offset 0;
    (depth, has, the scene's pixels at offset 0)"""
    rng = np.random.default_rng(seed)
    src = sr.texture(W + SHIFT * PERIOD, H, seed)
    x0, y0 = rng.uniform(16 + SHIFT * PERIOD, W - 16, n_kp), rng.uniform(16, H - 16, n_kp)
    level, angle = rng.integers(0, 3, n_kp).astype(np.int32), rng.uniform(0, 360, n_kp).astype(np.float32)
    depth = np.full((n_frames + n_kf, ctx.cells), -1.0)
    has = np.zeros((n_frames + n_kf, ctx.cells), np.uint8)
    for k in range(n_frames + n_kf):
        o = offset(k) if k < n_frames else 0
        ctx.upload_gray(k, np.ascontiguousarray(src[:, o:o + W]))
        ctx.build_pyramid(k, 1)
        ctx.describe_given_angle(k, np.stack([x0 - o, y0], 1), level, angle)
        has[k, :n_kp] = rng.uniform(size=n_kp) < 0.6
        depth[k, :n_kp] = np.where(has[k, :n_kp], Z, -1.0)
    ctx.set_keypoint_depths_batch(0, depth, has)
    return depth, has, np.stack([x0, y0], 1)


def old_route(ctx, slots, kf0, n_kf, kf, kfp_of, s, T, depth, has, K, p):
    """what a caller had to do before: fetch (the frames' slots and the keyframes' slots, each range at once), BoW, search, claim,
    orientation, edges, optimise"""
    n_frames = len(slots)
    kpf, kpk = ctx.get_keypoints_batch(0, n_frames), ctx.get_keypoints_batch(kf0, n_kf)
    ctx.compute_bow(0, n_frames, p.levelsup)
    ctx.compute_bow(kf0, n_kf, p.levelsup)
    kf_slots_of = (kf0 + kf).astype(np.int32)
    m12, _ = ctx.search_by_bow_slots(kf_slots_of, slots, th_low=p.th_low, knn_ratio=p.knn_ratio)
    claimed = np.full_like(m12, -1)
    for f in range(n_frames):
        n1, n2 = int(kpk["count"][kf[f]]), int(kpf["count"][f])
        m = np.where(kfp_of[f][:n1] >= 0, m12[f, :n1], -1)
        i = np.flatnonzero(m >= 0)
        holder = np.full(max(n2, 1), n1, np.int64)
        np.minimum.at(holder, m[i], i)
        keep = i[holder[m[i]] == i]
        claimed[f, keep] = m[keep]
    if p.check_orientation:
        _, _, ind = ctx.bow_orientation_slots(kf_slots_of, slots, claimed)
    off, X, obs, lvl, kind, status, points = [0], [], [], [], [], np.zeros(n_frames, np.int32), []
    for f in range(n_frames):
        a, b = int(kf[f]), int(slots[f])
        n1, n2 = int(kpk["count"][a]), int(kpf["count"][f])
        m = claimed[f, :n1]
        if p.check_orientation:
            bins = sk.rotation_bins(kpk["angle"][a, :n1], kpf["angle"][f, :n2], m)
            m = np.where((bins >= 0) & np.isin(bins, ind[f][ind[f] >= 0]), m, -1)
        kpp = sk.keypoint_points(m, kfp_of[f][:n1], n2)
        ur = sk.right_columns(kpf["px"][f, :n2], depth[b, :n2], sk.has_depth(depth[b, :n2], has[b, :n2]), p.baseline, K)
        j, x, ob, lv, kd = sk.edges(kpp, s["pw"], kpf["px"][f, :n2], ur, kpf["level"][f, :n2])
        status[f] = 1 if len(j) < p.min_matches else 0
        keep = slice(0, 0) if status[f] else slice(None)
        X.append(x[keep]); obs.append(ob[keep]); lvl.append(lv[keep]); kind.append(kd[keep]); off.append(off[-1] + len(lv[keep]))
        points.append(kpp)
    pose = ctx.default_pose_opt_params(baseline=p.baseline)
    r = ctx.optimize_pose_stereo(off, np.concatenate(X), np.concatenate(obs), np.concatenate(lvl), np.concatenate(kind), T, params=pose)
    status = np.where((status == 0) & (r["inliers"] < p.min_inliers), 2, status).astype(np.int32)
    return r["pose"], status, points


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "srk_bench.json")
    rows, same = {}, {}
    blob = fixtures.synthetic_vocabulary(k=10, L=5, seed=5)
    max_kf = max(1, max(FRAMES) // 32)
    for n_kp in KEYPOINTS:
        ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=max(FRAMES) + max_kf)
        assert ctx.cells == 3072
        ctx.vocab_load(blob)
        K = tuple(float(np.float32(getattr(ctx.params, k))) for k in ("fx", "fy", "cx", "cy"))
        depth, has, px = fill(ctx, max(FRAMES), max_kf, n_kp, 40 + n_kp)
        p = ctx.default_srk_params(levelsup=LEVELSUP)
        T_all = np.stack([[0, 0, 0, 1.0, -offset(k) * Z / K[0], 0, 0] for k in range(max(FRAMES))])
        # the scene's points under the keyframe's keypoints, 60 % of which carry theirs
        s = dict(pw=np.stack([(px[:, 0] - K[2]) / K[0] * Z, (px[:, 1] - K[3]) / K[1] * Z, np.full(n_kp, Z)], 1))
        row_kfp = np.full(ctx.cells, -1, np.int32)
        carry = np.random.default_rng(3).uniform(size=n_kp) < 0.6
        row_kfp[:n_kp][carry] = np.flatnonzero(carry)
        for n_frames in FRAMES:
            key = "%dx_kp%d" % (n_frames, n_kp)
            n_kf = max(1, n_frames // 32)
            slots, T = np.arange(n_frames, dtype=np.int32), T_all[:n_frames]
            kf_slot = (max(FRAMES) + np.arange(n_kf)).astype(np.int32)
            kf = (np.arange(n_frames) // 32 % n_kf).astype(np.int32)
            kf_point = np.tile(row_kfp, (n_kf, 1))
            args = ([s], kf_slot, np.zeros(n_kf, np.int32), kf_point, slots, kf, T)
            call = lambda: ctx.stereo_ref_keyframe_slots(*args, params=p, outputs=False)                  # noqa: E731
            got = ctx.stereo_ref_keyframe_slots(*args, params=p)
            route = lambda: old_route(ctx, slots, max(FRAMES), n_kf, kf, [row_kfp] * n_frames, s, T, depth, has, K, p)   # noqa: E731
            pose, status, points = route()
            same[key] = bool(pose.tobytes() == got["T_out"].tobytes() and np.array_equal(status, got["status"]) and
                             all(np.array_equal(q, got["kp_point"][f, :len(q)]) for f, q in enumerate(points)))
            c = got["counts"]
            row = dict(frames=n_frames, keyframes=n_kf, keypoints=n_kp, with_point=int(c[:, 1].sum()), search_matches=int(c[:, 4].sum()),
                       lost_claim=int(c[:, 5].sum()), removed_by_orientation=int(c[:, 6].sum()), edges=int(c[:, 7].sum()),
                       status_0=int((got["status"] == 0).sum()), inliers=int(got["inliers"].sum()), kernels={})
            for kern, launches in KERNELS.items():
                ms = []
                for k in range(3 + 20):
                    ctx.probe_begin(kern, 16)
                    call()
                    t, n = ctx.probe_end()
                    assert n == launches, (kern, n)
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
            row["call_all_outputs"] = timed(lambda: ctx.stereo_ref_keyframe_slots(*args, params=p), 2, 10)
            row["old_route"] = timed(route, *((WARMUP, TIMED) if n_frames <= 64 else (2, 10)))
            row["frames_per_second"] = n_frames / (row["call"]["median_ms"] * 1e-3)
            row["old_route_frames_per_second"] = n_frames / (row["old_route"]["median_ms"] * 1e-3)
            rows[key] = row
            print(key, json.dumps(row), "same" if same[key] else "DIFFERENT", flush=True)
        ctx.close()
    doc = dict(tool="tools/srk_bench.py", date=datetime.date.today().isoformat(), device=device_name(), warmup=WARMUP, timed=TIMED, rows=rows,
               bit_identical_to_old_route=same,
               note="kernels: HIP events around the launches of one kernel per run (k_srk_gather is launched twice); device_span: HIP events "
                    "around upload, launches and copy back; call: the Python binding's wall clock around the entry point with only T_out, status "
                    "and prior asked for; call_all_outputs: every output asked for; old_route: get_keypoints_batch, compute_bow, "
                    "search_by_bow_slots, numpy claim, bow_orientation_slots, numpy removal and edges, ygz_hip_optimize_pose_stereo")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    assert all(same.values()), same


if __name__ == "__main__":
    main()
