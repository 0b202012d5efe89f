#!/usr/bin/env python3
"""Call time of ygz_hip_search_by_projection (the projection-guided descriptor search, csrc/proj.hip) beside its restatement on one host core
(tests/proj_ref.c, gcc -O2), on the same inputs: seeded scenes of 1000 / 5000 / 20 000 points per problem against 1000 / 3072 keypoints, with
1, 2 and 16 problems per call, claim on; per row whether match, dist, pred_level and counts are bit-identical.  A shape above the call's
capacity (65 536 points over all problems) is recorded as refused.  Device: a host clock around each C ABI call, which ends in its one wait
(the arrays are marshalled once, outside the clock); 5 warm-up calls, then 50 timed; median / p10 / p90.  Restatement: the median of 3 runs.
Usage (on the GPU box): tools/proj_bench.py [out.json]; the default output is profiles/proj_bench.json."""
import ctypes as C
import datetime
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import proj_ref as pr                         # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402

W, H, L = 640, 480, 3


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def scene(n_pt, n_kp, seed):
    """tests/proj_ref.py's scene in array form (20 000 points at a time): three quarters of the points sit within a few pixels of a keypoint's
    ray at a compatible depth with its descriptor and about 0-70 flipped bits, the rest are anywhere; normals face the camera"""
    rng = np.random.default_rng(seed)
    K4 = pr.K4_DEFAULT
    S = pr.random_S(rng)
    R, t = pr.quat_to_R(S[:4]), S[4:7]
    kp_px = np.stack([rng.uniform(0, W, n_kp), rng.uniform(0, H, n_kp)], 1)
    kp_level = rng.integers(0, L, n_kp).astype(np.int32)
    kp_desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    stray = rng.uniform(size=n_pt) < 0.25
    j = rng.integers(0, n_kp, n_pt)
    px = np.where(stray[:, None], np.stack([rng.uniform(-60, W + 60, n_pt), rng.uniform(-60, H + 60, n_pt)], 1),
                  kp_px[j] + rng.uniform(-1, 1, (n_pt, 2)) * rng.choice([3.0, 9.0, 25.0], (n_pt, 1)))
    z = np.where(stray, rng.uniform(-2, 8, n_pt), rng.uniform(1.5, 7, n_pt))
    lv = np.minimum(kp_level[j] + rng.integers(0, 2, n_pt), L - 1)
    ratio = np.where(stray, 2.0 ** rng.uniform(-1.0, L + 0.5, n_pt), 2.0 ** lv * rng.uniform(0.55, 0.98, n_pt))
    flips = rng.uniform(size=(n_pt, 256)) < (rng.integers(0, 71, n_pt) / 256.0)[:, None]
    desc = np.where(stray[:, None], rng.integers(0, 256, (n_pt, 32)).astype(np.uint8), kp_desc[j] ^ np.packbits(flips, axis=1))
    Xc = np.stack([(px[:, 0] - K4[2]) / K4[0] * z, (px[:, 1] - K4[3]) / K4[1] * z, z], 1)
    d = np.linalg.norm(Xc, axis=1)
    nc = Xc / np.maximum(d, 1e-9)[:, None] + rng.normal(size=(n_pt, 3)) * 0.3
    nrm = (nc / np.linalg.norm(nc, axis=1)[:, None]) @ R * rng.uniform(0.7, 1.0, (n_pt, 1))
    return dict(kp_px=kp_px, kp_level=kp_level, kp_desc=kp_desc, pw=(Xc - t) @ R, pt_desc=desc, pt_dmax=ratio * d, pt_normal=nrm, S=S)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "proj_bench.json")
    ctx = _lib.HipContext(width=W, height=H, levels=L, max_frames=2)
    lib = ctx.lib
    ip = C.POINTER(C.c_int32)
    lib.ygz_hip_search_by_projection.argtypes = [C.c_void_p, C.c_int, C.POINTER(_lib.ProjProblem), C.POINTER(C.c_double), C.POINTER(_lib.ProjParams),
                                                 ip, ip, ip, ip]
    K = (C.c_double * 4)(*pr.K4_DEFAULT)
    prm = _lib.default_proj_params()
    rows = []
    for n_pt in (1000, 5000, 20000):
        for n_kp in (1000, 3072):
            base = [scene(n_pt, n_kp, 5000 + 17 * n_pt + n_kp + p) for p in range(2)]
            for P in (1, 2, 16):
                row = dict(n_pt=n_pt, n_kp=n_kp, problems=P, points=n_pt * P)
                rows.append(row)
                if n_pt * P > _lib.PROJ_MAX_POINTS:
                    try:
                        ctx.search_by_projection([base[0]] * P, pr.K4_DEFAULT)
                        row["refused"] = "accepted?"
                    except _lib.YgzHipError as e:
                        row["refused"] = "YGZ_E_CAPACITY" if e.code == _lib.E_CAPACITY else str(e.code)
                    print(json.dumps(row), flush=True)
                    continue
                scs = [base[p % 2] if p < 2 else dict(base[p % 2], S=pr.random_S(np.random.default_rng(p))) for p in range(P)]
                arr, keep = _lib.proj_problems(scs)
                N = n_pt * P
                match, dist, pred = (np.zeros(N, np.int32) for _ in range(3))
                counts = np.zeros((P, 2), np.int32)
                dev = []
                for k in range(55):
                    t0 = time.perf_counter()
                    rc = lib.ygz_hip_search_by_projection(ctx._ctx, P, arr, K, C.byref(prm), match.ctypes.data_as(ip), dist.ctypes.data_as(ip),
                                                          pred.ctypes.data_as(ip), counts.ctypes.data_as(ip))
                    t1 = time.perf_counter()
                    assert rc == 0, rc
                    if k >= 5:
                        dev.append(t1 - t0)
                host = []
                for k in range(3):
                    t0 = time.perf_counter()
                    ref = pr.search(scs, w=W, h=H, L=L)
                    host.append(time.perf_counter() - t0)
                same = all(np.array_equal(a, ref[k]) for a, k in ((match, "match"), (dist, "dist"), (pred, "pred_level"), (counts, "counts")))
                row.update(device=stats(dev), one_core_ms=float(np.median(host) * 1e3), bit_identical=bool(same),
                           matches=int(counts[:, 0].sum()), overflowed=int(counts[:, 1].sum()), searched=int((pred >= 0).sum()))
                row["one_core_over_device"] = row["one_core_ms"] / row["device"]["median_ms"]
                print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/proj_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               image=[W, H], levels=L, params=dict(th=prm.th, th_dist=prm.th_dist, claim=prm.claim), warmup=5, timed=50, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
