#!/usr/bin/env python3
"""Times of the stereo pose optimisation (csrc/popt.hip) on 512 frames of 1000 edges each -- half of them stereo, 10 % gross outliers, the entry
pose 2 degrees and 5 cm off (16 distinct frames of tests/popt_ref.py's generator, repeated) -- beside ygz_hip_optimize_pose_only, the library's
monocular per-frame refinement, on the same frames in the same run: that is the call a stereo tracker would otherwise make.  One
ygz_hip_optimize_pose_stereo call over all frames per run, with the library's default parameters: the whole call by HIP events on the context's
stream (packed upload, the kernel, copy back), k_pose_opt and k_pose_only_ba by the context's kernel probe.  5 warm-up runs, then 30 timed;
median (p10 - p90).  The first and the last frame are compared with the restatement (tests/popt_ref.c) bit for bit, and the restatement's trial
trace of the distinct frames gives the number of passes a frame makes.  Usage (on the GPU box): tools/popt_bench.py [out.json]; the default
output is profiles/popt_bench.json."""
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import popt_ref as pr                         # noqa: E402  (test infrastructure: the restatement and the scene generator)
from ygz_slam_amd import _lib                 # noqa: E402

FRAMES, DISTINCT, EDGES, OUTLIERS = 512, 16, 1000, 0.10
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


def axis_angle(pose7):
    """[t; log(so3)] of ygz_hip_optimize_pose_only from qx qy qz qw tx ty tz"""
    v, w = pose7[:3], pose7[3]
    s = np.linalg.norm(v)
    aa = np.zeros(3) if s == 0 else 2.0 * np.arctan2(s, w) * v / s
    return np.concatenate([pose7[4:], aa])


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "popt_bench.json")
    distinct = [pr.make_frame(900 + q, EDGES, outliers=OUTLIERS) for q in range(DISTINCT)]
    frames = [distinct[q % DISTINCT] for q in range(FRAMES)]
    a = pr.pack(frames)
    ctx = _lib.HipContext(width=pr.WIDTH, height=pr.HEIGHT, levels=pr.LEVELS, max_frames=1)
    p = ctx.default_pose_opt_params(baseline=pr.BASELINE)
    stereo = lambda: ctx.optimize_pose_stereo(a["frame_off"], a["pw"], a["obs"], a["level"], a["kind"], a["poses"], params=p)
    px, entry = np.ascontiguousarray(a["obs"][:, :2]), np.stack([axis_angle(f.pose) for f in frames])
    mono = lambda: ctx.optimize_pose_only(a["frame_off"], px, a["pw"], entry)
    t_call, t_kernel = events(ctx, stereo), probe(ctx, "k_pose_opt", stereo)
    t_mono_call, t_mono_kernel = events(ctx, mono), probe(ctx, "k_pose_only_ba", mono)
    got, got_mono = stereo(), mono()
    ctx.close()
    same, passes = True, []
    q0 = pr.defaults()
    for q in (0, FRAMES - 1):
        want = pr.optimize(frames[q], q0)
        lo, hi = a["frame_off"][q], a["frame_off"][q + 1]
        same = same and got["pose"][q].tobytes() == want["pose"].tobytes() and np.array_equal(got["outlier"][lo:hi], want["outlier"])
        same = same and got["chi2"][lo:hi].tobytes() == want["chi2"].tobytes() and got["cost_final"][q].tobytes() == want["cost_final"].tobytes()
    for f in distinct:
        r = pr.optimize(f, q0)
        evaluated = sum(1 for _, _, c in r["trace"] if c != pr.TRIAL_FAILED)
        passes.append(dict(linearisations=int(r["lm_iterations"].sum()), cost_passes=evaluated, classifications=r["rounds_run"]))
    truth_err = [float(np.linalg.norm(got["pose"][q][4:] - frames[q].truth[4:])) for q in range(DISTINCT)]
    flags_ok = all(np.array_equal(got["outlier"][a["frame_off"][q]:a["frame_off"][q + 1]].astype(bool), frames[q].is_outlier) for q in range(DISTINCT))
    rows = dict(optimize_pose_stereo_call=stats(t_call), k_pose_opt=stats(t_kernel), optimize_pose_only_call=stats(t_mono_call),
                k_pose_only_ba=stats(t_mono_kernel))
    rows["kernel_to_pose_only_kernel"] = rows["k_pose_opt"]["median_ms"] / rows["k_pose_only_ba"]["median_ms"]
    rows["call_to_pose_only_call"] = rows["optimize_pose_stereo_call"]["median_ms"] / rows["optimize_pose_only_call"]["median_ms"]
    doc = dict(tool="tools/popt_bench.py", date=datetime.date.today().isoformat(), device=device_name(), frames=FRAMES, distinct_frames=DISTINCT,
               edges_per_frame=EDGES, stereo_edges=int((a["kind"] == 2).sum()), gross_outliers=int(sum(f.is_outlier.sum() for f in frames)),
               bit_identical=bool(same), flags_equal_truth=bool(flags_ok), inliers_mean=float(got["inliers"].mean()),
               rounds_run_mean=float(got["rounds_run"].mean()), lm_iterations_per_frame=float(got["lm_iterations"].sum(axis=1).mean()),
               passes_per_distinct_frame=passes, translation_error_m_max=max(truth_err),
               pose_only_inliers_mean=float(got_mono[3].mean()), pose_only_rounds_mean=float(got_mono[4].mean()),
               upload_bytes=int(a["pw"].nbytes + a["obs"].nbytes + a["level"].nbytes + a["kind"].nbytes + a["poses"].nbytes + a["frame_off"].nbytes),
               warmup=WARMUP, timed=TIMED, rows=rows)
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
