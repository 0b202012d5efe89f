#!/usr/bin/env python3
"""Call time of ygz_hip_pose_graph_optimize (the Sim3 pose-graph optimiser, csrc/pgo.hip) beside two host yardsticks on the same graphs: its
restatement on one host core (tests/pgo_ref.c, gcc -O2), and a host Levenberg-Marquardt of the same rules that solves every step directly with
scipy.sparse (J from the restatement's blocks, (J^T J + lambda I) d = b by spsolve; its total includes the Python marshalling of the
linearisation and the retraction, so the time inside spsolve alone is recorded beside it).  Graphs: tests/pgo_ref.py's rings with 25 % chords and
the loop scene's drift, N = 16, 128 and 1024, measurement noise 0.001.  Per row: whether the device is bit-identical to the restatement, the LM
iterations, the solves and the CG iterations per solve.  Device: a host clock around each C ABI call, which ends in its one wait (the arrays are
marshalled once, outside the clock); 5 warm-up calls, then 50 timed (fewer when 50 would take more than a minute, never fewer than 5); median /
p10 / p90.  Restatement: the median of 3 runs (1 run at N = 1024).  Usage (on the GPU box): tools/pgo_bench.py [out.json]; the default
output is profiles/pgo_bench.json."""
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
import pgo_ref as pg                          # noqa: E402  (test infrastructure: the one-core restatement)
from ygz_slam_amd import _lib                 # noqa: E402


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), p10_ms=float(np.percentile(ts, 10)), p90_ms=float(np.percentile(ts, 90)), calls=len(ts))


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:                         # noqa: BLE001
        return "unknown"


def sparse_lm(g, max_iterations=20, max_trials=10, min_rel_decrease=1e-9):
    """the restatement's outer loop with every step solved directly: -> (final cost, LM iterations, solves, seconds inside spsolve)"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    S = np.array(g["S"], float)
    free = np.flatnonzero(np.asarray(g["fixed"]) == 0)
    col = -np.ones(len(S), int)
    col[free] = np.arange(len(free))
    edges = np.asarray(g["edges"])
    E = len(edges)
    rows = (7 * np.arange(E)[:, None, None] + np.arange(7)[None, :, None]) + np.zeros((1, 1, 7), int)
    lam, ni, solves, its, t_solve = 0.0, 2.0, 0, 0, 0.0
    chi = None
    for it in range(max_iterations):
        lin = pg.linearize(dict(g, S=S))
        chi = lin["cost"]
        blocks, rr, cc = [], [], []
        for side, J in ((0, lin["Ji"]), (1, lin["Jj"])):
            keep = col[edges[:, side]] >= 0
            cols = 7 * col[edges[keep, side]][:, None, None] + np.arange(7)[None, None, :] + np.zeros((1, 7, 1), int)
            blocks.append(J[keep].ravel()); rr.append(rows[keep].ravel()); cc.append(cols.ravel())
        J = sp.csr_matrix((np.concatenate(blocks), (np.concatenate(rr), np.concatenate(cc))), shape=(7 * E, 7 * len(free)))
        H = (J.T @ J).tocsc()
        b = -(J.T @ lin["res"].ravel())
        if it == 0:
            lam = 1e-5 * H.diagonal().max()
        rho, q, converged = 0.0, 0, False
        while True:
            t0 = time.perf_counter()
            x = spsolve(H + lam * sp.identity(H.shape[0], format="csc"), b)
            t_solve += time.perf_counter() - t0
            solves += 1
            Sn = S.copy()
            ok = True
            for k, v in enumerate(free):
                o, Sn[v] = pg.retract(S[v], x[7 * k:7 * k + 7])
                ok = ok and bool(o)
            tmp = pg.linearize(dict(g, S=Sn))["cost"] if ok else np.inf
            rho = (chi - tmp) / (x @ (lam * x + b) + 1e-3)
            if ok and rho > 0 and np.isfinite(tmp):
                lam *= min(max(1 - (2 * rho - 1) ** 3, 1 / 3), 2 / 3)
                ni = 2.0
                converged = chi - tmp <= min_rel_decrease * chi
                chi, S = tmp, Sn
            else:
                lam *= ni
                ni *= 2
            q += 1
            if not (rho < 0 and q < max_trials):
                break
        its += 1
        if q == max_trials or rho == 0 or converged:
            break
    return chi, its, solves, t_solve


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pgo_bench.json")
    ctx = _lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    lib = ctx.lib
    _lib.pgo_argtypes(lib)
    prm = _lib.default_pgo_params()
    rows = []
    sparse_lm(pg.ring(4, seed=1))             # loads scipy.sparse outside the clocks
    for n in (16, 128, 1024):
        g = pg.ring(n, chords=n // 4, noise=0.001, seed=n)
        S, fixed, edges, M = _lib.pgo_arrays(g["S"], g["fixed"], g["edges"], g["M"])
        So, res = np.zeros_like(S), _lib.PgoResult()
        dp = C.POINTER(C.c_double)
        args = (ctx._ctx, len(S), S.ctypes.data_as(dp), fixed.ctypes.data_as(C.POINTER(C.c_uint8)), len(edges),
                edges.ctypes.data_as(C.POINTER(C.c_int32)), M.ctypes.data_as(dp), C.byref(prm), So.ctypes.data_as(dp), C.byref(res))
        dev, spent = [], 0.0
        for k in range(55):
            t0 = time.perf_counter()
            rc = lib.ygz_hip_pose_graph_optimize(*args)
            t1 = time.perf_counter()
            assert rc == 0, rc
            if k >= 5:
                dev.append(t1 - t0)
                spent += t1 - t0
                if spent > 60.0 and len(dev) >= 5:
                    break
        host = []
        for k in range(1 if n >= 1024 else 3):
            t0 = time.perf_counter()
            ref = pg.optimize(g)
            host.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        s_cost, s_its, s_solves, t_spsolve = sparse_lm(g)
        t_sparse = time.perf_counter() - t0
        same = np.array_equal(ref["S"].view(np.uint64), So.view(np.uint64)) and all(
            getattr(res, k) == ref[k] for k in ("status", "lm_iterations", "n_solves", "cg_iterations_total", "cg_capped", "cost_initial",
                                                "cost_final", "lambda_"))
        row = dict(vertices=n, edges=len(edges), unknowns=7 * int((fixed == 0).sum()), device=stats(dev),
                   one_core_ms=float(np.median(host) * 1e3), sparse_direct_ms=t_sparse * 1e3, bit_identical=bool(same), status=res.status,
                   lm_iterations=res.lm_iterations, solves=res.n_solves, cg_iterations=res.cg_iterations_total, cg_capped=res.cg_capped,
                   cg_per_solve=res.cg_iterations_total / max(res.n_solves, 1), cost_initial=res.cost_initial, cost_final=res.cost_final,
                   sparse_direct=dict(cost_final=float(s_cost), lm_iterations=s_its, solves=s_solves, spsolve_ms=t_spsolve * 1e3))
        row["device_us_per_cg_iteration"] = 1e3 * row["device"]["median_ms"] / max(res.cg_iterations_total, 1)
        row["one_core_over_device"] = row["one_core_ms"] / row["device"]["median_ms"]
        row["sparse_direct_over_device"] = row["sparse_direct_ms"] / row["device"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    doc = dict(tool="tools/pgo_bench.py", date=datetime.date.today().isoformat(), device=device_name(), host=platform.processor() or platform.machine(),
               params=dict(max_iterations=prm.max_iterations, max_trials=prm.max_trials, cg_max_iterations=prm.cg_max_iterations,
                           cg_tol=prm.cg_tol, min_rel_decrease=prm.min_rel_decrease), warmup=5, timed=50, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
