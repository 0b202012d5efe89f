#!/usr/bin/env python3
"""Call times of the resident map (csrc/rmap.hip) on the scene of tools/lmt_bench.py: its eight resident frames and its
map of 200 keyframes and 20000 points (make_map, the same generator and seed), with what the selection needs added by tools/lms_bench.py's
rules: the features of a keyframe numbered in a random order with gaps, ten covisible neighbours per keyframe, and frames of ENTRIES entries
of which 800 carry points seen from within three keyframes of a random centre (frames_on).  max_keyframes 80, max_points 8192.  Batches of 1,
8, 64 and 512 frames, identity entry poses.

Per batch:  (a) the existing route, everything inside the clock: ygz_hip_local_map_select, ygz_hip_map_point_attributes, the host filter
(numpy: mask, cumulative sum, prior re-basing) and ygz_hip_stereo_local_map_indexed;  (b) ygz_hip_stereo_local_map_resident with the map
already uploaded;  (c) every kernel of (b) from the context's kernel probe (HIP events around its launches; 2 warm-up and 10 timed runs per
kernel).  T_out and status of (a) and (b) are compared on bits.  At one frame also section 35's baseline A: ygz_hip_stereo_local_map_slots on
the one host-gathered filtered set, the gather outside the clock.  Once:  (d) ygz_hip_map_upload alone;  (e) ygz_hip_map_update of 1000
points (positions) with 10 centres.  The clock stands around the Python binding with outputs=False (T_out and status alone come back from
the tracking calls) and arrays already in the ABI's types.  Not timed: the object-graph gather of a host class.  3 warm-up calls, then 20
timed; median / p10 / p90.  Usage (on the GPU box): tools/rmap_bench.py [out.json]; default profiles/rmap_bench.json."""
import datetime
import json
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lmt_bench as lb                        # noqa: E402  (the scene, the clock)
import lms_bench as sb                        # noqa: E402  (the frames' entries)
from ygz_slam_amd import _lib                 # noqa: E402

K, N_POINTS, SLOTS = lb.K, lb.N_POINTS, lb.SLOTS
N_COV, MAX_KF, MAX_PT = sb.N_COV, sb.MAX_KF, sb.MAX_PT
FRAMES = [1, 8, 64, 512]
KERNELS = ["k_lms_vote", "k_lms_points", "k_lms_place", "k_lms_prior", "k_rmap_filter", "k_slm_index", "k_slm_gather", "k_strack_search",
           "k_slm_resolve", "k_pose_opt", "k_slm_scatter"]
UPDATE_POINTS, UPDATE_CENTRES = 1000, 10


def selection_side(rng, kf):
    """tools/lms_bench.py's rules on the observations of lmt_bench's map: distinct feature indices per keyframe in a random order with gaps;
    ten covisible neighbours, nearest index first"""
    feat = np.zeros(len(kf), np.int32)
    for k in range(K):
        at = np.flatnonzero(kf == k)
        feat[at] = rng.permutation(2 * len(at))[:len(at)]
    cov = np.zeros((K, N_COV), np.int32)
    for k in range(K):
        cov[k] = sorted((c for c in range(K) if c != k), key=lambda c: (abs(c - k), c))[:N_COV]
    return feat, cov


def host_filter(sel, state, cells, fr_off):
    """steps 2 to 4 on the host, vectorised: (list_pt [F, MP], list_len [F], prior [F, cells])"""
    lp, n_pt = sel["local_pt"], sel["n_pt"]
    F, MP = lp.shape
    inside = np.arange(MP)[None, :] < n_pt[:, None]
    keep = inside & (state[np.maximum(lp, 0)] == 1)
    pos = np.cumsum(keep, axis=1) - 1
    moved = np.where(keep, pos, -1).astype(np.int32)
    out = np.full((F, MP), -1, np.int32)
    rows = np.nonzero(keep)
    out[rows[0], pos[rows]] = lp[rows]
    prior = np.full((F, cells), -1, np.int32)
    for f in range(F):
        at = sel["fr_prior"][fr_off[f]:fr_off[f + 1]]
        prior[f, :len(at)] = np.where(at >= 0, moved[f, np.maximum(at, 0)], -1)
    return out, keep.sum(axis=1).astype(np.int32), prior


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rmap_bench.json")
    rng = np.random.default_rng(31)
    ctx = _lib.HipContext(width=lb.W, height=lb.H, levels=3, max_frames=SLOTS)
    counts = lb.resident_frames(ctx, rng)
    m = lb.make_map(rng)
    center, pw, off, kf, level = m["center"], m["pw"], m["off"], m["kf"], m["level"]
    desc = rng.integers(0, 256, (N_POINTS, 32)).astype(np.uint8)
    feat, cov = selection_side(rng, kf)
    kf_bad, pt_bad = np.zeros(K, np.uint8), np.zeros(N_POINTS, np.uint8)
    sb.ENTRIES = min(sb.ENTRIES, ctx.cells)
    arrays = dict(kf_bad=kf_bad, cov=cov, n_cov=N_COV, offsets=off, kf=kf, feat=feat, pt_bad=pt_bad, centre=center, a_offsets=off, a_kf=kf,
                  a_level=level, pw=pw, pt_desc=desc, pt_has_desc=None)
    rmap = ctx.map_create()
    att = rmap.upload(arrays)
    upload = lb.stats(lb.timed(lambda: rmap.upload(arrays, outputs=False)))
    pi = rng.permutation(N_POINTS)[:UPDATE_POINTS].astype(np.int32)
    ci = rng.permutation(K)[:UPDATE_CENTRES].astype(np.int32)
    new_pw, new_c = np.ascontiguousarray(pw[pi]), np.ascontiguousarray(center[ci])
    update = lb.stats(lb.timed(lambda: rmap.update(pi, new_pw, c_idx=ci, centre=new_c)))                  # the same values: the map does not move
    info = rmap.info()
    once = dict(keyframes=K, points=N_POINTS, observations=int(len(kf)), resident_bytes=info["resident_bytes"], upload=upload,
                update=dict(points=UPDATE_POINTS, centres=UPDATE_CENTRES, call=update),
                upload_kernel=lb.probe(ctx, "k_mpa_attr", lambda: rmap.upload(arrays, outputs=False)),
                update_kernels={k: lb.probe(ctx, k, lambda: rmap.update(pi, new_pw, c_idx=ci, centre=new_c)) for k in ("k_rmap_scatter", "k_mpa_attr")})
    print(json.dumps(once), flush=True)
    I = np.array([0, 0, 0, 1.0, 0, 0, 0])
    lms = dict(max_keyframes=MAX_KF, max_points=MAX_PT)
    rows = []
    for F in FRAMES:
        fr_off, fr_pt = sb.frames_on(rng, F, m["start"], m["n_obs"])
        slots, li, T = (np.arange(F) % SLOTS).astype(np.int32), np.arange(F, dtype=np.int32), np.tile(I, (F, 1))

        def existing():
            sel = ctx.local_map_select(kf_bad, cov, off, kf, feat, fr_off, fr_pt, pt_bad, outputs=("n_pt", "local_pt", "fr_prior"), **lms)
            a = ctx.map_point_attributes(center, pw, off, kf, level)
            lp, ll, prior = host_filter(sel, a["state"], ctx.cells, fr_off)
            pts = dict(pw=pw, pt_desc=desc, pt_dmax=a["dmax"], pt_normal=a["normal"])
            return ctx.stereo_local_map_indexed(pts, lp, ll, slots, li, T, prior, outputs=False), lp, ll, prior, a

        resident = lambda: ctx.stereo_local_map_resident(rmap, slots, T, fr_off, fr_pt, lms=lms, outputs=False)   # noqa: E731
        (want, lp, ll, prior, a), got = existing(), resident()
        same = all(np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), np.ascontiguousarray(want[k]).view(np.uint8)) for k in ("T_out", "status"))
        kernels = {kern: lb.probe(ctx, kern, resident) for kern in KERNELS}
        row = dict(frames=F, entries=int(sb.ENTRIES), list_length_mean=float(ll.mean()), stride=MAX_PT, keypoints_mean=float(counts.mean()),
                   bit_identical=bool(same), optimised=int((got["status"] == 0).sum()), existing=lb.stats(lb.timed(lambda: existing())),
                   resident=dict(call=lb.stats(lb.timed(resident)), kernels=kernels, kernels_ms=sum(v["median_ms"] for v in kernels.values())))
        row["speedup"] = row["existing"]["median_ms"] / row["resident"]["call"]["median_ms"]
        if F == 1:
            n = int(ll[0])
            one = {k: np.ascontiguousarray(v[lp[0, :n]]) for k, v in dict(pw=pw, pt_desc=desc, pt_dmax=a["dmax"], pt_normal=a["normal"]).items()}
            row["by_value_one_set"] = lb.stats(lb.timed(lambda: ctx.stereo_local_map_slots([one], slots, [0], T, prior, outputs=False)))
        row["frames_per_upload_to_break_even"] = (upload["median_ms"] / max(row["existing"]["median_ms"] - row["resident"]["call"]["median_ms"], 1e-9) * F
                                                  if row["speedup"] > 1 else None)
        rows.append(row)
        print(json.dumps(row), flush=True)
    rmap.destroy()
    ctx.close()
    doc = dict(tool="tools/rmap_bench.py", date=datetime.date.today().isoformat(), device=lb._lib_device(), host=platform.processor() or platform.machine(),
               warmup=lb.WARMUP, timed=lb.TIMED, map=once, rows=rows, refused_points=int((att["state"] != 1).sum()),
               note="existing: select + attributes + numpy filter + indexed tracking, all inside one host clock; resident: the one call on the "
                    "uploaded map; calls through the Python binding with outputs=False; kernels: HIP events around the launches of each kernel, "
                    "one kernel per run; by_value_one_set: ygz_hip_stereo_local_map_slots on the one filtered set gathered on the host, the "
                    "gather outside the clock (section 35's baseline A); frames_per_upload_to_break_even: upload median / (existing - resident) "
                    "per frame of the batch; not timed: the object-graph gather of a host class")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    assert all(r["bit_identical"] for r in rows)


if __name__ == "__main__":
    main()
