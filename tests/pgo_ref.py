"""ctypes loader of tests/pgo_ref.c, the restatement of the Sim3 pose-graph optimiser (ygz_slam_amd/csrc/pgo.hip) that tests/test_pgo_ref.py
and tests/test_gpu_pgo.py hold ygz_hip_pose_graph_optimize against.  Test infrastructure: compiled with gcc into a temporary directory the
first time it is used, never imported by the package.  Also the seeded graph generators of the tests: rings with chords, stars, a per-edge
drift, measurement noise, a component whose residual is exactly zero."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

FAILED, CONVERGED, MAX_ITERATIONS, STALLED = 0, 1, 2, 3
LANES = 256
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1], np.float64)


class PgParams(ctypes.Structure):
    """the layout of ygz_pgo_params (include/ygz_hip.h)"""
    _fields_ = [("max_iterations", ctypes.c_int32), ("max_trials", ctypes.c_int32), ("cg_max_iterations", ctypes.c_int32),
                ("fix_scale", ctypes.c_int32), ("cg_tol", ctypes.c_double), ("min_rel_decrease", ctypes.c_double)]


class PgResult(ctypes.Structure):
    """the layout of ygz_pgo_result"""
    _fields_ = [("cost_initial", ctypes.c_double), ("cost_final", ctypes.c_double), ("lambda_", ctypes.c_double), ("status", ctypes.c_int32),
                ("lm_iterations", ctypes.c_int32), ("n_solves", ctypes.c_int32), ("cg_iterations_total", ctypes.c_int32),
                ("cg_capped", ctypes.c_int32), ("pad", ctypes.c_int32)]


DEFAULTS = dict(max_iterations=20, max_trials=10, cg_max_iterations=0, fix_scale=0, cg_tol=1e-8, min_rel_decrease=1e-9)
RESULT_FIELDS = ("cost_initial", "cost_final", "lambda_", "status", "lm_iterations", "n_solves", "cg_iterations_total", "cg_capped")


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="pgo_ref_")
        so = os.path.join(d, "libpgo_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "pgo_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
    return _lib


def _d(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.reshape(shape) if shape else a


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(**kw):
    p = PgParams()
    for k, v in dict(DEFAULTS, **kw).items():
        setattr(p, k, v)
    return p


def compose(A, B):
    o = np.zeros(8)
    lib().pg_compose(_p(_d(A)), _p(_d(B)), _p(o))
    return o


def inverse(S):
    o = np.zeros(8)
    lib().pg_inverse(_p(_d(S)), _p(o))
    return o


def retract(S, x):
    """-> (ok, Delta(x) o S)"""
    o = np.zeros(8)
    ok = lib().pg_retract(_p(_d(S)), _p(_d(x)), _p(o))
    return ok, o


def delta(x):
    """Delta(x) as a similarity"""
    ok, o = retract(IDENTITY, x)
    assert ok
    return o


def lift(E):
    r = np.zeros(7)
    ok = lib().pg_lift(_p(_d(E)), _p(r))
    return ok, r


def edge_terms(Si, Sj, M, fix_scale=False):
    """-> (ok, r [7], Ji [7][7], Jj [7][7])"""
    r, Ji, Jj = np.zeros(7), np.zeros((7, 7)), np.zeros((7, 7))
    ok = lib().pg_edge_terms(_p(_d(Si)), _p(_d(Sj)), _p(_d(M)), int(fix_scale), _p(r), _p(Ji), _p(Jj))
    return ok, r, Ji, Jj


def residual(Si, Sj, M):
    E, r = np.zeros(8), np.zeros(7)
    ok = lib().pg_edge_residual(_p(_d(Si)), _p(_d(Sj)), _p(_d(M)), _p(E), _p(r))
    return ok, r


def _graph(g):
    S, M = _d(g["S"], (-1, 8)), _d(g["M"], (-1, 8))
    fixed = np.ascontiguousarray(g["fixed"], dtype=np.uint8)
    edges = np.ascontiguousarray(g["edges"], dtype=np.int32).reshape(-1, 2)
    return S, fixed, edges, M


def linearize(g, fix_scale=False):
    """-> dict(ok, res [E][7], Ji, Jj [E][7][7], cost) at g's estimate"""
    S, fixed, edges, M = _graph(g)
    E = len(edges)
    res, Ji, Jj, cost = np.zeros((E, 7)), np.zeros((E, 7, 7)), np.zeros((E, 7, 7)), ctypes.c_double()
    ok = lib().pg_linearize(len(S), _p(S), E, _p(edges, ctypes.c_int32), _p(M), int(fix_scale), _p(res), _p(Ji), _p(Jj), ctypes.byref(cost))
    return dict(ok=ok, res=res, Ji=Ji, Jj=Jj, cost=cost.value)


def optimize(g, **kw):
    """the whole call: dict(S [N][8], and the fields of the result block)"""
    S, fixed, edges, M = _graph(g)
    p, r, out = params(**kw), PgResult(), np.zeros_like(S)
    lib().pg_optimize(len(S), _p(S), _p(fixed, ctypes.c_uint8), len(edges), _p(edges, ctypes.c_int32), _p(M), ctypes.byref(p), _p(out),
                      ctypes.byref(r))
    d = dict((k, getattr(r, k)) for k in RESULT_FIELDS)
    d["S"] = out
    return d


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def _axis_angle(axis, deg):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([np.sin(h) * a, [np.cos(h)]])


def sim3(axis, deg, t, s=1.0):
    return np.concatenate([_axis_angle(axis, deg), np.asarray(t, float), [s]])


def ring_truth(n, radius=3.0):
    """n cameras on a circle (world -> camera, scale 1), each turned by 360 / n degrees against the last"""
    T = []
    for i in range(n):
        a = 360.0 * i / n
        T.append(sim3([0.1, 1.0, 0.05], a, [radius * np.cos(np.deg2rad(a)) - radius, 0.05 * i, radius * np.sin(np.deg2rad(a))]))
    return np.array(T)


def ring(n, chords=0, drift=(1.2, 4.0, 0.1), noise=0.0, seed=0, fixed=(0,)):
    """a ring of n vertices whose odometry edges (k -> k + 1) each carry 1 / (n - 1) of the drift (scale, degrees, metres), the estimate
    integrated along them from the truth at vertex 0, `chords` edges between random non-neighbours measured on the estimate, and the exact
    loop edge n - 1 -> 0 from the truth.  noise: sigma of a Delta on every measurement but the loop edge's"""
    rng = np.random.default_rng(seed)
    T = ring_truth(n)
    m = max(n - 1, 1)
    D = sim3([0.3, 1.0, -0.2], drift[1] / m, np.array([0.6, -0.3, 0.74]) * drift[2] / m, drift[0] ** (1.0 / m))
    S, edges, M = [T[0]], [], []
    for k in range(n - 1):
        Mk = compose(D, compose(T[k + 1], inverse(T[k])))
        S.append(compose(Mk, S[k]))
        edges.append((k, k + 1)); M.append(Mk)
    S = np.array(S)
    done = set()
    while len(done) < chords:
        i, j = sorted(rng.choice(n, 2, replace=False))
        if j - i < 2 or (i, j) == (0, n - 1) or (i, j) in done:
            continue
        done.add((i, j))
        edges.append((i, j)); M.append(compose(S[j], inverse(S[i])))
    if noise > 0:
        M = [compose(delta(rng.normal(0, noise, 7)), Mk) for Mk in M]
    edges.append((n - 1, 0)); M.append(compose(T[0], inverse(T[n - 1])))
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    return dict(S=S, fixed=fx, edges=np.array(edges, np.int32), M=np.array(M), truth=T)


def consistent(n, kind="ring", seed=0, perturb=(5.0, 0.1, 0.1), fixed=(0,)):
    """exact measurements from a ground truth with scales in e^+-0.3; the estimate is the truth moved by up to `perturb` (degrees, metres,
    log scale) at every free vertex.  kind: "ring" (k -> k + 1 and n - 1 -> 0) or "star" (vertex 0 to every other one)"""
    rng = np.random.default_rng(seed)
    T = np.array([sim3(rng.normal(size=3), rng.uniform(0, 60), rng.uniform(-2, 2, 3), np.exp(rng.uniform(-0.3, 0.3))) for _ in range(n)])
    edges = [(k, (k + 1) % n) for k in range(n)] if kind == "ring" else [(0, k) if k % 2 else (k, 0) for k in range(1, n)]
    M = np.array([compose(T[j], inverse(T[i])) for i, j in edges])
    fx = np.zeros(n, np.uint8)
    fx[list(fixed)] = 1
    S = T.copy()
    for v in range(n):
        if fx[v]:
            continue
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * 2 * np.tan(np.deg2rad(rng.uniform(0, perturb[0])) / 2)
        S[v] = compose(delta(np.concatenate([w, rng.uniform(-perturb[1], perturb[1], 3), [0.0]])), T[v])
        S[v][7] = T[v][7] * np.exp(rng.uniform(-perturb[2], perturb[2]))
    return dict(S=S, fixed=fx, edges=np.array(edges, np.int32), M=M, truth=T)


def with_zero_component(g, n=3):
    """g plus a free component of n vertices without rotation, with integer translations and scale 1, and exact measurements between them:
    every residual there is exactly zero"""
    N = len(g["S"])
    S = [np.array([0, 0, 0, 1, 1.0 + k, 2.0 * k, -3.0 + k, 1.0]) for k in range(n)]
    edges = [(N + k, N + (k + 1) % n) for k in range(n if n > 2 else n - 1)]
    M = [compose(S[j - N], inverse(S[i - N])) for i, j in edges]
    out = dict(g)
    out["S"] = np.concatenate([g["S"], S]); out["M"] = np.concatenate([g["M"], M])
    out["edges"] = np.concatenate([g["edges"], np.array(edges, np.int32)]); out["fixed"] = np.concatenate([g["fixed"], np.zeros(n, np.uint8)])
    if "truth" in g:
        out["truth"] = np.concatenate([g["truth"], S])
    return out
