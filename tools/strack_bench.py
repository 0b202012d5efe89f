#!/usr/bin/env python3
"""Kernel and call time of the stereo tracking search (csrc/strack.hip) at the per-frame shapes.  Workloads: the frame-to-frame search, 1
problem x 1000 points of the last frame, and the local-map search, 1 problem x 2000 and x 8000 local points, each at 1000 and at 3072
keypoints of the current frame (3072 = ygz_hip_max_keypoints at 640 x 480); scenes of tests/strack_ref.py (60 % of the keypoints with a right
column).  k_strack_search comes from the context's kernel probe (HIP events around the launch), the device span from HIP events around
upload, launch and copy back, the call from the host clock around the whole entry point (the Python binding's array packing and the host
walk included): 5 warm-up runs, then 50 timed; median (p10 - p90).  Beside them ygz_hip_search_by_projection (csrc/proj.hip: no right column,
no second best) on the LOCAL shapes with the window of the wide factor, and the restatement's C code (tests/strack_ref.c) alone on one host
core (1 warm-up, 5 timed).  Every output is compared with the restatement bit for bit in the same run.  No time is fixed in advance: the file
records what was measured and on which device.  Usage (on the GPU box): tools/strack_bench.py [out.json]; the default output is
profiles/strack_bench.json."""
import ctypes
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import strack_ref as st                       # noqa: E402  (test infrastructure: the restatement)
from ygz_slam_amd import _lib                 # noqa: E402

WARMUP, TIMED = 5, 50
SHAPES = [("frame", st.FRAME, 1000), ("local", st.LOCAL, 2000), ("local", st.LOCAL, 8000)]
KEYPOINTS = [1000, 3072]
NAMES = st.INT_OUTPUTS + ("proj", "cand", "counts", "rot")


def stats(ms):
    ms = np.asarray(ms)
    return dict(median_ms=float(np.median(ms)), p10_ms=float(np.percentile(ms, 10)), p90_ms=float(np.percentile(ms, 90)), runs=len(ms))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def measure(ctx, call, kernel=None):
    kernel_ms, span_ms, call_ms = [], [], []
    for k in range(WARMUP + TIMED):
        if kernel:
            ctx.probe_begin(kernel, 16)
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        if kernel:
            t, n = ctx.probe_end()
            assert n == 1, (kernel, n)
        if k >= WARMUP:
            call_ms.append((t1 - t0) * 1e3)
            if kernel:
                kernel_ms.append(t)
    for k in range(WARMUP + TIMED):           # the device span in runs of its own: the two event pairs do not share a run
        ctx.timer_begin()
        call()
        t = ctx.timer_end()
        if k >= WARMUP:
            span_ms.append(t)
    out = dict(device_span=stats(span_ms), call=stats(call_ms))
    if kernel:
        out["kernel"] = stats(kernel_ms)
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "strack_bench.json")
    K4 = st.K4_DEFAULT
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2, intrinsics=K4)
    assert ctx.cells == 3072
    p = ctx.default_strack_params()
    rows, same = {}, {}
    for name, mode, n_pt in SHAPES:
        for n_kp in KEYPOINTS:
            key = "%s_1x%d_kp%d" % (name, n_pt, n_kp)
            if mode == st.FRAME:
                sets, pbs = st.frame_scene(n_pt, n_kp, 900 + n_kp + n_pt, direction=1)
            else:
                sets, pbs = st.local_scene(n_pt, n_kp, 900 + n_kp + n_pt, th=1.0)
            got = ctx.stereo_track_search(sets, pbs, K4, params=p)
            ref = st.search(sets, pbs, K4, 640, 480, 3)
            same[key] = bool(all(got[k].tobytes() == ref[k].tobytes() for k in NAMES))
            row = measure(ctx, lambda: ctx.stereo_track_search(sets, pbs, K4, params=p), "k_strack_search")
            row["pairs"], row["searched"], row["matches"] = int(len(ref["match"])), int(ref["counts"][:, 1].sum()), int(ref["counts"][:, 0].sum())
            row["overflowed"], row["gated_candidates"], row["candidates"] = int(ref["counts"][:, 2].sum()), int(ref["n_gated"].sum()), int(ref["n_cand"].sum())
            if mode == st.LOCAL:
                # the nearest existing call on the same shape: no right column, no second best; the wide factor as its window
                pp = [dict(sets[0], S=np.concatenate([b["T"], [1.0]]), **{k: b[k] for k in ("kp_px", "kp_level", "kp_desc")}) for b in pbs]
                row["search_by_projection"] = measure(ctx, lambda: ctx.search_by_projection(pp, K4, th=4.0, th_dist=100, claim=1))
            # the restatement's C code alone: structs and outputs made once, outside the clock
            sa, pa, keep = st.c_arrays(sets, pbs)
            N = len(ref["match"])
            o = [np.zeros(N, np.int32) for _ in range(7)]
            proj, cand, counts, rot = np.zeros((N, 3)), np.zeros((N, 8), np.int32), np.zeros((1, 4), np.int32), np.zeros((1, 33), np.int32)
            rp, k4 = st.params(), np.ascontiguousarray(K4, np.float64)
            ip, dp, L = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), st.lib()
            ms = []
            for k in range(1 + 5):
                t0 = time.perf_counter()
                L.st_search(1, sa, 1, pa, k4.ctypes.data_as(dp), 640, 480, 3, ctypes.byref(rp), *[a.ctypes.data_as(ip) for a in o],
                            proj.ctypes.data_as(dp), cand.ctypes.data_as(ip), counts.ctypes.data_as(ip), rot.ctypes.data_as(ip))
                if k >= 1:
                    ms.append((time.perf_counter() - t0) * 1e3)
            row["restatement_one_core"] = stats(ms)
            rows[key] = row
            print(key, json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/strack_bench.py", date=datetime.date.today().isoformat(), device=device_name(), warmup=WARMUP, timed=TIMED, rows=rows,
               bit_identical=same,
               note="kernel: HIP events around the launch; device_span: HIP events around upload, launch and copy back; call: the Python binding's "
                    "wall clock around the entry point, its array packing and the host walk included; restatement: the C function alone, 1 warm-up "
                    "and 5 timed runs")
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
