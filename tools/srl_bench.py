#!/usr/bin/env python3
"""Kernel, device and call time of the stereo relocalisation on resident slots (csrc/srl.hip) at 1, 8 and 64 lost frames of a 640 x 480
sequence, each with 5 candidate keyframes and 1000 keypoints, 60 % of them with a depth.  The frames are windows of one texture that move by
3 pixels per frame, back and forth, every frame in a slot of its own; the keypoints move with the pictures.  Five keyframes, each in a slot
of its own: the first shows an unrelated texture (it fails at the search), the second the scene with a set whose points are moved one by one
(it fails at the PnP), the other three the scene at offset 0 with the true set; 60 % of a keyframe's keypoints carry the scene's point under
them.  Every frame gets the five in that order, so the third wins.  The vocabulary is synthetic (k = 10, L = 5) and levelsup is 3, so that
the FeatureVector has the about 100 nodes an ORB vocabulary of six levels has at levelsup 4.

Per shape: every kernel of the call from the context's kernel probe (HIP events around its launches; 3 warm-up and 20 timed runs per
kernel), the device span from HIP events around upload, launches and copy back, and the call from the host clock around the whole entry point
(5 warm-up, 50 timed; median, p10 - p90), asking for T_out, best, status, T_opt and prior only and asking for every output; a call takes 256
problems, so the 64 frames go in two calls of 32 frames and every figure of that shape is the sum of the two.  Beside it the
staged route through the entry points a caller has had so far, on host arrays: ygz_hip_get_keypoints_batch for all slots, per frame and
candidate ygz_hip_bow_transform of both descriptor sets and ygz_hip_search_by_bow, the claim, the rotation bins and the association lists in
numpy, ONE ygz_hip_pnp_ransac per chunk of 64 problems, the edge lists in numpy, ONE ygz_hip_optimize_pose_stereo, the winner in Python
(5 warm-up and 50 timed runs at 1 frame, 2 and 10 at 8, 1 and 3 at 64).  The depths are taken as already on the host there.  best, status,
T_pnp and T_opt of the two routes are compared bit for bit in the same run.  No time is fixed in advance: the file records what was measured
and on which device.  Usage (on the GPU box): tools/srl_bench.py [out.json]; the default output is profiles/srl_bench.json."""
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
FRAMES = [1, 8, 64]
N_KP, N_KF = 1000, 5
LEVELSUP = 3
KERNELS = {"k_srl_gather": 2, "k_bow_transform": 1, "k_bow_match": 1, "k_srl_resolve": 1, "k_srl_sets": 1, "k_pnp_solve": 1, "k_pnp_score": 1,
           "k_pnp_select": 1, "k_srl_edges": 1, "k_pose_opt": 1, "k_srl_scatter": 1, "k_srl_pick": 1}      # launches per call


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
    o = 1 + k % (2 * PERIOD - 2)
    return (o if o < PERIOD else 2 * PERIOD - o) * SHIFT


def fill(ctx, n_frames, seed):
    """frame k = the texture's window at offset(k), its keypoints the scene's points at that offset; behind them the keyframes at offset 0,
    the first on another texture; (depth, has, the scene's pixels at offset 0)"""
    rng = np.random.default_rng(seed)
    src, other = sr.texture(W + SHIFT * PERIOD, H, seed), sr.texture(W + SHIFT * PERIOD, H, seed + 1)
    x0, y0 = rng.uniform(16 + SHIFT * PERIOD, W - 16, N_KP), rng.uniform(16, H - 16, N_KP)
    level, angle = rng.integers(0, 3, N_KP).astype(np.int32), rng.uniform(0, 360, N_KP).astype(np.float32)
    depth = np.full((n_frames + N_KF, ctx.cells), -1.0)
    has = np.zeros((n_frames + N_KF, ctx.cells), np.uint8)
    for k in range(n_frames + N_KF):
        o = offset(k) if k < n_frames else 0
        ctx.upload_gray(k, np.ascontiguousarray((other if k == n_frames else src)[:, o:o + W]))
        ctx.build_pyramid(k, 1)
        ctx.describe_given_angle(k, np.stack([x0 - o, y0], 1), level, angle)
        has[k, :N_KP] = rng.uniform(size=N_KP) < 0.6
        depth[k, :N_KP] = np.where(has[k, :N_KP], Z, -1.0)
    ctx.set_keypoint_depths_batch(0, depth, has)
    return depth, has, np.stack([x0, y0], 1)


def staged_route(ctx, n_frames, kf0, sets, kf_set, row_kfp, depth, has, K, p):
    """what a caller has had so far: fetch, per problem the two BoW transforms and the search on host arrays, claim, orientation and
    associations in numpy, the PnP of all problems (64 per call), the edges in numpy, one pose optimisation, the winner"""
    kpf, kpk = ctx.get_keypoints_batch(0, n_frames), ctx.get_keypoints_batch(kf0, N_KF)
    K4 = np.array(K, np.float64)
    probs = []
    for f in range(n_frames):
        n2 = int(kpf["count"][f])
        d2 = kpf["desc"][f, :n2]
        node2 = ctx.bow_transform(d2, p.levelsup)[2]
        ur = sk.right_columns(kpf["px"][f, :n2], depth[f, :n2], sk.has_depth(depth[f, :n2], has[f, :n2]), p.baseline, K)
        for k in range(N_KF):
            n1 = int(kpk["count"][k])
            kfp = row_kfp[:n1]
            node1 = sk.masked_nodes(ctx.bow_transform(kpk["desc"][k, :n1], p.levelsup)[2], kfp)
            found = ctx.search_by_bow(kpk["desc"][k, :n1], node1, d2, node2, th_low=p.th_low, knn_ratio=p.knn_ratio)[0].astype(np.int32)
            _, lost = sk.claim(found, n2)
            m = np.where(lost, -1, found).astype(np.int32)
            if p.check_orientation:
                bins = sk.rotation_bins(kpk["angle"][k, :n1], kpf["angle"][f, :n2], m)
                hist = np.bincount(bins[bins >= 0], minlength=30)[:30].astype(np.int32)
                ind = top3(hist)
                m = np.where((bins >= 0) & np.isin(bins, ind[ind >= 0]), m, -1).astype(np.int32)
            kpp = sk.keypoint_points(m, kfp, n2)
            j, X, obs, lvl, kind = sk.edges(kpp, sets[kf_set[k]]["pw"], kpf["px"][f, :n2], ur, kpf["level"][f, :n2])
            probs.append(dict(j=j, X=X, obs=obs, lvl=lvl, kind=kind))
    P = len(probs)
    status = np.array([1 if len(q["j"]) < p.min_matches else 0 for q in probs], np.int32)
    T_pnp = np.tile(sk.IDENTITY, (P, 1))
    masks = [np.zeros(len(q["j"]), bool) for q in probs]
    live = np.flatnonzero(status == 0)
    for c0 in range(0, len(live), _lib.PNP_MAX_PROBLEMS):
        chunk = live[c0:c0 + _lib.PNP_MAX_PROBLEMS]
        off = np.concatenate([[0], np.cumsum([len(probs[q]["j"]) for q in chunk])]).astype(np.int32)
        res, inl = ctx.pnp_ransac(np.concatenate([probs[q]["X"] for q in chunk]), np.concatenate([probs[q]["obs"][:, :2] for q in chunk]), off, K4,
                                  max_iter=p.pnp.max_iter, chi2=p.pnp.chi2, min_inliers=p.pnp.min_inliers)
        for i, q in enumerate(chunk):
            T_pnp[q] = res[i]["T_cw"]
            masks[q] = np.asarray(inl[off[i]:off[i + 1]], bool)
            if not res[i]["success"]:
                status[q] = 2
    off, X, obs, lvl, kind = [0], [], [], [], []
    for q, pr in enumerate(probs):
        e = np.flatnonzero(masks[q]) if status[q] == 0 else np.zeros(0, np.int64)
        X.append(pr["X"][e]); obs.append(pr["obs"][e]); lvl.append(pr["lvl"][e]); kind.append(pr["kind"][e]); off.append(off[-1] + len(e))
    pose = ctx.default_pose_opt_params(baseline=p.baseline)
    r = ctx.optimize_pose_stereo(off, np.concatenate(X), np.concatenate(obs), np.concatenate(lvl), np.concatenate(kind), T_pnp, params=pose)
    status = np.where((status == 0) & (r["inliers"] < p.min_final_inliers), 3, status).astype(np.int32)
    best = np.full(n_frames, -1, np.int32)
    for f in range(n_frames):
        ok = np.flatnonzero(status[f * N_KF:(f + 1) * N_KF] == 0)
        if len(ok):
            best[f] = f * N_KF + ok[0]
    return best, status, T_pnp, r["pose"]


def top3(hist):
    """the three maxima of the rotation histogram as yo_bow_orientation takes them (csrc/slot_pose_dev.h: ygz_rot_top3)"""
    max1 = max2 = max3 = 0
    i0 = i1 = i2 = -1
    for b in range(30):
        s = int(hist[b])
        if s > max1:
            max3, max2, max1, i2, i1, i0 = max2, max1, s, i1, i0, b
        elif s > max2:
            max3, max2, i2, i1 = max2, s, i1, b
        elif s > max3:
            max3, i2 = s, b
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        i1 = i2 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        i2 = -1
    return np.array([i0, i1, i2], np.int32)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "srl_bench.json")
    rows, same = {}, {}
    blob = fixtures.synthetic_vocabulary(k=10, L=5, seed=5)
    for n_frames in FRAMES:
        ctx = _lib.HipContext(width=W, height=H, levels=3, max_frames=n_frames + N_KF)
        ctx.vocab_load(blob)
        K = tuple(float(np.float32(getattr(ctx.params, k))) for k in ("fx", "fy", "cx", "cy"))
        depth, has, px = fill(ctx, n_frames, 1040)
        p = ctx.default_srl_params(levelsup=LEVELSUP)
        true = dict(pw=np.stack([(px[:, 0] - K[2]) / K[0] * Z, (px[:, 1] - K[3]) / K[1] * Z, np.full(N_KP, Z)], 1))
        moved = dict(pw=true["pw"] + np.random.default_rng(4).uniform(-1.0, 1.0, true["pw"].shape))
        sets, kf_set = [true, moved], np.array([0, 1, 0, 0, 0], np.int32)
        row_kfp = np.full(ctx.cells, -1, np.int32)
        carry = np.random.default_rng(3).uniform(size=N_KP) < 0.6
        row_kfp[:N_KP][carry] = np.flatnonzero(carry)
        key = "%dx%d_kp%d" % (n_frames, N_KF, N_KP)
        slots = np.arange(n_frames, dtype=np.int32)
        kf_slot = (n_frames + np.arange(N_KF)).astype(np.int32)
        cands = [list(range(N_KF))] * n_frames
        # a call takes YGZ_SRL_MAX_PROBLEMS = 256 problems: 64 frames of 5 candidates go in two calls of 32 frames
        per_call = min(n_frames, 32)
        chunks = [(sets, kf_slot, kf_set, np.tile(row_kfp, (N_KF, 1)), slots[a:a + per_call], cands[a:a + per_call])
                  for a in range(0, n_frames, per_call)]
        assert all(len(c[4]) * N_KF <= _lib.SRL_MAX_PROBLEMS for c in chunks)
        call = lambda: [ctx.stereo_relocalize_slots(*a, params=p, outputs=False) for a in chunks]     # noqa: E731
        full = lambda: [ctx.stereo_relocalize_slots(*a, params=p) for a in chunks]                     # noqa: E731
        parts = full()
        got = {k: np.concatenate([q[k] for q in parts]) for k in ("status", "T_pnp", "T_opt", "counts")}
        got["best"] = np.concatenate([np.where(q["best"] >= 0, q["best"] + i * per_call * N_KF, -1) for i, q in enumerate(parts)]).astype(np.int32)
        route = lambda: staged_route(ctx, n_frames, n_frames, sets, kf_set, row_kfp, depth, has, K, p)                      # noqa: E731
        best, status, T_pnp, T_opt = route()
        same[key] = bool(np.array_equal(best, got["best"]) and np.array_equal(status, got["status"]) and
                         T_pnp.tobytes() == got["T_pnp"].tobytes() and T_opt.tobytes() == got["T_opt"].tobytes())
        c = got["counts"]
        row = dict(frames=n_frames, calls=len(chunks), candidates=N_KF, problems=n_frames * N_KF, keypoints=N_KP, associations=int(c[:, 7].sum()),
                   pnp_inliers=int(c[:, 8].sum()), final_inliers=int(c[:, 9].sum()), relocalised=int((got["best"] >= 0).sum()),
                   status=[int((got["status"] == s).sum()) for s in range(4)], kernels={})
        for kern, launches in KERNELS.items():
            ms = []
            for k in range(3 + 20):
                ctx.probe_begin(kern, 16)
                call()
                t, n = ctx.probe_end()
                assert n == launches * len(chunks), (kern, n)
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
        row["call_all_outputs"] = timed(full, 2, 10)
        row["staged_route"] = timed(route, *{1: (WARMUP, TIMED), 8: (2, 10)}.get(n_frames, (1, 3)))
        row["frames_per_second"] = n_frames / (row["call"]["median_ms"] * 1e-3)
        row["staged_route_frames_per_second"] = n_frames / (row["staged_route"]["median_ms"] * 1e-3)
        rows[key] = row
        print(key, json.dumps(row), "same" if same[key] else "DIFFERENT", flush=True)
        ctx.close()
    doc = dict(tool="tools/srl_bench.py", date=datetime.date.today().isoformat(), device=device_name(), warmup=WARMUP, timed=TIMED, rows=rows,
               bit_identical_to_staged_route=same,
               note="kernels: HIP events around the launches of one kernel per run (k_srl_gather is launched twice per call); calls: 64 frames of 5 "
                    "candidates are two calls of 32 frames, every figure their sum; device_span: HIP events "
                    "around upload, launches and copy back; call: the Python binding's wall clock around the entry point with only T_out, best, "
                    "status, T_opt and prior asked for; call_all_outputs: every output asked for; staged_route: get_keypoints_batch, per problem "
                    "two ygz_hip_bow_transform and one ygz_hip_search_by_bow on host arrays, numpy claim, orientation and associations, "
                    "ygz_hip_pnp_ransac per 64 problems, numpy edges, one ygz_hip_optimize_pose_stereo, the winner in Python")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    assert all(same.values()), same


if __name__ == "__main__":
    main()
