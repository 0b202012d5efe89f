"""ctypes loader of tests/sba_ref.c, the restatement of the stereo bundle adjustment (ygz_slam_amd/csrc/sba.hip) that tests/test_sba_ref.py and
tests/test_gpu_sba.py hold ygz_hip_stereo_ba against.  Test infrastructure: compiled with gcc into a temporary directory the first time it
is used, never imported by the package.  Also the seeded scene generator of the tests and of tools/sba_bench.py (gba_ref.scene's rings with
pyramid levels, stereo columns, level-scaled noise and gross outliers) and the numpy witness of the round logic: the same spec written
another way -- vectorised residuals, Jacobians by central differences through the retraction, one dense solve of the whole damped system
instead of the Schur complement and conjugate gradients, np.sum for the sums."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import gba_ref as gb

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

FAILED, CONVERGED, MAX_ITERATIONS, STALLED = 0, 1, 2, 3
MAX_ROUNDS = 4
K4 = gb.K4
BASELINE = 0.1
CHI2_MONO, CHI2_STEREO = 5.991, 7.815


class SbParams(ctypes.Structure):
    """the layout of ygz_sba_params (include/ygz_hip.h)"""
    _fields_ = [("max_iterations", ctypes.c_int32), ("max_trials", ctypes.c_int32), ("cg_max_iterations", ctypes.c_int32),
                ("cg_batch", ctypes.c_int32), ("cg_tol", ctypes.c_double), ("min_rel_decrease", ctypes.c_double), ("baseline", ctypes.c_double),
                ("chi2_mono", ctypes.c_double), ("chi2_stereo", ctypes.c_double), ("rounds", ctypes.c_int32), ("robust_rounds", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 4)]


class SbResult(ctypes.Structure):
    """the layout of ygz_sba_result"""
    _fields_ = [("cost_initial", ctypes.c_double * 4), ("cost_final", ctypes.c_double * 4), ("lambda_", ctypes.c_double * 4),
                ("rounds_run", ctypes.c_int32), ("launches", ctypes.c_int32), ("status", ctypes.c_int32 * 4), ("lm_iterations", ctypes.c_int32 * 4),
                ("n_solves", ctypes.c_int32 * 4), ("cg_iterations", ctypes.c_int32 * 4), ("cg_capped", ctypes.c_int32 * 4),
                ("inliers", ctypes.c_int32 * 4)]


class SbProblem(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int), ("nl", ctypes.c_int), ("ne", ctypes.c_int), ("poses", ctypes.POINTER(ctypes.c_double)),
                ("points", ctypes.POINTER(ctypes.c_double)), ("obs", ctypes.POINTER(ctypes.c_double)), ("fixed", ctypes.POINTER(ctypes.c_uint8)),
                ("edge_pose", ctypes.POINTER(ctypes.c_int32)), ("edge_point", ctypes.POINTER(ctypes.c_int32)),
                ("kind", ctypes.POINTER(ctypes.c_uint8)), ("level", ctypes.POINTER(ctypes.c_int32)), ("fx", ctypes.c_double), ("fy", ctypes.c_double),
                ("cx", ctypes.c_double), ("cy", ctypes.c_double)]


DEFAULTS = dict(max_iterations=10, max_trials=10, cg_max_iterations=0, cg_batch=0, cg_tol=1e-8, min_rel_decrease=1e-9, baseline=0.0,
                chi2_mono=CHI2_MONO, chi2_stereo=CHI2_STEREO, rounds=2, robust_rounds=1, iterations=(5, 10, 0, 0))
ROUND_FIELDS = ("cost_initial", "cost_final", "lambda_", "status", "lm_iterations", "n_solves", "cg_iterations", "cg_capped", "inliers")


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="sba_ref_")
        so = os.path.join(d, "libsba_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "sba_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        _lib.sb_weight.restype = ctypes.c_double
    return _lib


_d, _p = gb._d, gb._p


def params(**kw):
    p = SbParams()
    for k, v in dict(DEFAULTS, **kw).items():
        if k == "iterations":
            v = list(v) + [0] * (4 - len(v))
            for i in range(4):
                p.iterations[i] = int(v[i])
        else:
            setattr(p, k, v)
    return p


def arrays(g):
    """the arrays of a problem dict in the ABI's types: gba_ref.arrays' with obs [E][3], then kind [E] uint8 and level [E] int32"""
    return (_d(g["poses"], (-1, 7)), np.ascontiguousarray(g["fixed"], np.uint8).reshape(-1), _d(g["points"], (-1, 3)),
            np.ascontiguousarray(g["edge_pose"], np.int32).reshape(-1), np.ascontiguousarray(g["edge_point"], np.int32).reshape(-1),
            _d(g["obs"], (-1, 3)), np.ascontiguousarray(g["kind"], np.uint8).reshape(-1), np.ascontiguousarray(g["level"], np.int32).reshape(-1))


def _problem(g):
    poses, fixed, points, ep, el, obs, kind, level = a = arrays(g)
    K = g.get("K", K4)
    pb = SbProblem(len(poses), len(points), len(ep), _p(poses), _p(points), _p(obs), _p(fixed, ctypes.c_uint8), _p(ep, ctypes.c_int32),
                   _p(el, ctypes.c_int32), _p(kind, ctypes.c_uint8), _p(level, ctypes.c_int32), K[0], K[1], K[2], K[3])
    return pb, a


def call_params(g, **kw):
    """the parameters a scene is run with: its baseline, then the caller's"""
    return dict(dict(baseline=g.get("baseline", BASELINE)), **kw)


def edge_terms(T, X, ob, kind, level=0, K=K4, bf=K4[0] * BASELINE, robust=0):
    """-> (ok, r [3], weight, rho, Jp [3][6], Jl [3][3])"""
    r, w, rho, Jp, Jl = np.zeros(3), ctypes.c_double(), ctypes.c_double(), np.zeros((3, 6)), np.zeros((3, 3))
    d2 = CHI2_STEREO if kind == 2 else CHI2_MONO
    ok = lib().sb_edge_terms(_p(_d(T)), _p(_d(X)), _p(_d(ob)), _p(_d(K)), ctypes.c_double(bf), int(kind), int(level), int(robust),
                             ctypes.c_double(d2), ctypes.c_double(np.sqrt(d2)), _p(r), ctypes.byref(w), ctypes.byref(rho), _p(Jp), _p(Jl))
    return ok, r, w.value, rho.value, Jp, Jl


def linearize(g, **kw):
    """-> dict(ok, res [E][3], w [E], Jp [E][3][6], Jl [E][3][3], Hpp [N][21], bp [N][6], Hll [L][6], bl [L][3], cost) at g's estimate"""
    pb, keep = _problem(g)
    N, L, E = pb.n, pb.nl, pb.ne
    p = params(**call_params(g, **kw))
    o = dict(res=np.zeros((E, 3)), w=np.zeros(E), Jp=np.zeros((E, 3, 6)), Jl=np.zeros((E, 3, 3)), Hpp=np.zeros((N, 21)), bp=np.zeros((N, 6)),
             Hll=np.zeros((L, 6)), bl=np.zeros((L, 3)))
    cost = ctypes.c_double()
    ok = lib().sb_linearize(ctypes.byref(pb), ctypes.byref(p), _p(o["res"]), _p(o["w"]), _p(o["Jp"]), _p(o["Jl"]), _p(o["Hpp"]), _p(o["bp"]),
                            _p(o["Hll"]), _p(o["bl"]), ctypes.byref(cost))
    del keep
    o.update(ok=bool(ok), cost=cost.value)
    return o


def optimize(g, **kw):
    """the whole call: dict(poses [N][7], points [L][3], outlier [E], chi2 [E], rounds_run and the per-round arrays of the result block)"""
    pb, keep = _problem(g)
    p, r = params(**call_params(g, **kw)), SbResult()
    poses, points, outlier, chi2 = np.zeros((pb.n, 7)), np.zeros((pb.nl, 3)), np.zeros(pb.ne, np.uint8), np.zeros(pb.ne)
    lib().sb_optimize(ctypes.byref(pb), ctypes.byref(p), _p(poses), _p(points), _p(outlier, ctypes.c_uint8), _p(chi2), ctypes.byref(r))
    del keep
    d = dict((k, np.array(getattr(r, k))) for k in ROUND_FIELDS)
    d.update(rounds_run=r.rounds_run, launches=r.launches, poses=poses, points=points, outlier=outlier, chi2=chi2)
    return d


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
def scene(n_poses, n_points, obs_per_point=3, stereo="half", outliers=0.0, seed=0, fixed=(0,), rings=1, levels=4, noise=0.5, baseline=BASELINE,
          perturb=(0.01, 0.02, 0.02), repeat_edge=False):
    """gba_ref.scene's cameras, points, edges and perturbed start; every edge gets a pyramid level (cycling 0 .. levels - 1 in edge order), a
    kind -- stereo "all", "none" or "half" (edges alternate) -- and uR = u - bf / z from the truth; Gaussian noise of sigma noise x 2^level on
    all three coordinates; a fraction `outliers` of the edges displaced by 20 to 60 pixels of the edge's level in (u, v), uR moving with u"""
    g = gb.scene(n_poses, n_points, obs_per_point, noise=0.0, outliers=0.0, perturb=perturb, seed=seed, fixed=fixed, rings=rings,
                 repeat_edge=repeat_edge)
    rng = np.random.default_rng(seed + 100003)
    E = len(g["edge_pose"])
    level = (np.arange(E) % levels).astype(np.int32)
    kind = {"all": np.full(E, 2), "none": np.full(E, 1), "half": 1 + (np.arange(E) % 2)}[stereo].astype(np.uint8)
    bf = g["K"][0] * baseline
    obs = np.zeros((E, 3))
    for e in range(E):
        px, z = gb.project(g["truth_poses"][g["edge_pose"][e]], g["truth_points"][g["edge_point"][e]])
        obs[e] = [px[0], px[1], px[0] - bf / z]
    if noise > 0:
        obs += rng.normal(0, 1, (E, 3)) * (noise * 2.0 ** level)[:, None]
    bad = np.zeros(E, bool)
    if outliers > 0:
        idx = rng.choice(E, int(round(outliers * E)), replace=False)
        ang, mag = rng.uniform(0, 2 * np.pi, len(idx)), rng.uniform(20, 60, len(idx)) * 2.0 ** level[idx]
        obs[idx, 0] += mag * np.cos(ang); obs[idx, 1] += mag * np.sin(ang); obs[idx, 2] += mag * np.cos(ang)
        bad[idx] = True
    del g["huber"]
    g.update(obs=obs, kind=kind, level=level, baseline=baseline, displaced=bad)
    return g


def as_gba(g):
    """the mono, level-0 reading of a gba_ref problem: obs [E][3] with uR = 0, every kind 1, every level 0"""
    E = len(g["edge_pose"])
    s = dict(g)
    s.update(obs=np.concatenate([np.asarray(g["obs"], float).reshape(-1, 2), np.zeros((E, 1))], axis=1), kind=np.ones(E, np.uint8),
             level=np.zeros(E, np.int32), baseline=0.0)
    return s


# ---- the numpy witness -----------------------------------------------------------------------------------------------------------------
def _retract_all(T, d):
    """gb_retract for rows: T [M][7], d [M][6]"""
    dq = np.concatenate([0.5 * d[:, :3], np.ones((len(d), 1))], axis=1)
    dq /= np.linalg.norm(dq, axis=1)[:, None]
    ax, ay, az, aw = dq.T
    bx, by, bz, bw = T[:, :4].T
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                  aw * bw - ax * bx - ay * by - az * bz], axis=1)
    q /= np.linalg.norm(q, axis=1)[:, None]
    t = np.einsum("mij,mj->mi", _rot_all(dq), T[:, 4:]) + d[:, 3:]
    return np.concatenate([q, t], axis=1)


def _rot_all(q):
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)


class Witness:
    def __init__(self, g, **kw):
        self.T0, self.fixed, self.X0, self.ep, self.el, self.obs, self.kind, self.level = arrays(g)
        self.K = g.get("K", K4)
        self.p = dict(DEFAULTS, **call_params(g, **kw))
        self.bf = self.K[0] * self.p["baseline"]
        self.w = 0.25 ** self.level.astype(float)
        self.d2 = np.where(self.kind == 2, self.p["chi2_stereo"], self.p["chi2_mono"])
        self.free = np.flatnonzero(self.fixed == 0)
        self.col = np.full(len(self.T0), -1)
        self.col[self.free] = 6 * np.arange(len(self.free))

    def residuals(self, Te, Xe):
        """per edge from the edge's own pose row and point row: r [E][3] (zero third row for mono), defined [E]"""
        K, bf = self.K, self.bf
        with np.errstate(all="ignore"):
            P = np.einsum("eij,ej->ei", _rot_all(Te[:, :4]), Xe) + Te[:, 4:]
            z = P[:, 2]
            u = K[0] * (P[:, 0] / z) + K[2]
            r = np.stack([self.obs[:, 0] - u, self.obs[:, 1] - (K[1] * (P[:, 1] / z) + K[3]),
                          np.where(self.kind == 2, self.obs[:, 2] - (u - bf / z), 0.0)], axis=1)
            ok = (z > 0) & np.isfinite(r).all(axis=1)
        return np.where(ok[:, None], r, 0.0), ok

    def chi2(self, r):
        return self.w * np.sum(r * r, axis=1)

    def cost(self, T, X, active, robust):
        r, ok = self.residuals(T[self.ep], X[self.el])
        c = self.chi2(r)
        rho = c.copy()
        if robust:
            out = c > self.d2
            rho[out] = 2 * np.sqrt(c[out]) * np.sqrt(self.d2[out]) - self.d2[out]
        good = bool(np.all(ok[active]))
        total = float(np.sum(rho[active]))
        return total, good and np.isfinite(total), r, c

    def system(self, T, X, active, robust):
        """the dense normal equations over (free poses, points) at (T, X): H, b"""
        E, h = len(self.ep), 1e-6
        Te, Xe = T[self.ep], X[self.el]
        r, _ = self.residuals(Te, Xe)
        c = self.chi2(r)
        wt = self.w.copy()
        if robust:
            out = c > self.d2
            wt[out] *= np.sqrt(self.d2[out]) / np.sqrt(c[out])
        wt = np.where(active, wt, 0.0)
        J = np.zeros((E, 3, 9))
        for k in range(6):
            d = np.zeros((E, 6))
            d[:, k] = h
            J[:, :, k] = (self.residuals(_retract_all(Te, d), Xe)[0] - self.residuals(_retract_all(Te, -d), Xe)[0]) / (2 * h)
        for k in range(3):
            d = np.zeros((E, 3))
            d[:, k] = h
            J[:, :, 6 + k] = (self.residuals(Te, Xe + d)[0] - self.residuals(Te, Xe - d)[0]) / (2 * h)
        nv = 6 * len(self.free) + 3 * len(X)
        H, b = np.zeros((nv, nv)), np.zeros(nv)
        for e in np.flatnonzero(active):
            cp, cl = self.col[self.ep[e]], 6 * len(self.free) + 3 * self.el[e]
            idx = np.concatenate([np.arange(cp, cp + 6) if cp >= 0 else [], np.arange(cl, cl + 3)]).astype(int)
            Je = J[e][:, 6 if cp < 0 else 0:]
            H[np.ix_(idx, idx)] += wt[e] * Je.T @ Je
            b[idx] -= wt[e] * Je.T @ r[e]
        return H, b

    def apply(self, T, X, dx):
        Tn, Xn = T.copy(), X + dx[6 * len(self.free):].reshape(-1, 3)
        if len(self.free):
            Tn[self.free] = _retract_all(T[self.free], dx[:6 * len(self.free)].reshape(-1, 6))
        return Tn, Xn

    def classify(self, T, X):
        r, ok = self.residuals(T[self.ep], X[self.el])
        c = np.where(ok, self.chi2(r), 0.0)
        out = (~ok | (c > self.d2)) & (self.kind != 0)
        return out.astype(np.uint8), np.where(self.kind == 0, -1.0, c)

    def run(self):
        p = self.p
        T, X = self.T0.copy(), self.X0.copy()
        outlier = np.zeros(len(self.ep), np.uint8)
        o = dict(status=np.zeros(4, int), lm_iterations=np.zeros(4, int), inliers=np.zeros(4, int), cost_initial=np.zeros(4), cost_final=np.zeros(4),
                 margins=[])
        for k in range(p["rounds"]):
            active = (self.kind != 0) & ~((k > 0) & (outlier != 0))
            robust = k < p["robust_rounds"]
            lam, ni, cur, status = 0.0, 2.0, 0.0, MAX_ITERATIONS
            for it in range(p["iterations"][k]):
                cost, ok, _, _ = self.cost(T, X, active, robust)
                if it == 0:
                    if not ok:
                        status = FAILED
                        break
                    o["cost_initial"][k] = cost
                cur = cost
                H, b = self.system(T, X, active, robust)
                if it == 0:
                    lam, ni = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0
                rho, qmax, converged = 0.0, 0, False
                while True:
                    temp, scale, ok = np.finfo(float).max, 0.0, True
                    with np.errstate(all="ignore"):
                        try:
                            A = H + lam * np.eye(len(b))
                            np.linalg.cholesky(A)
                            dx = np.linalg.solve(A, b)
                            ok = bool(np.isfinite(dx).all())
                        except np.linalg.LinAlgError:
                            ok = False
                    if ok:
                        Tn, Xn = self.apply(T, X, dx)
                        scale = float(np.sum(dx * (lam * dx + b)))
                        temp, ok, _, _ = self.cost(Tn, Xn, active, robust)
                        if not ok:
                            temp, scale = np.finfo(float).max, 0.0
                    with np.errstate(all="ignore"):
                        rho = (cur - temp) / (scale + 1e-3)
                    if not np.isfinite(rho):
                        rho = -1.0
                    if ok and rho > 0:
                        lam *= max(1 / 3, min(2 / 3, 1 - (2 * rho - 1) ** 3))
                        ni = 2.0
                        converged = cur - temp <= p["min_rel_decrease"] * cur
                        cur, T, X = temp, Tn, Xn
                    else:
                        lam, ni = lam * ni, ni * 2
                        if not np.isfinite(lam):
                            break
                    qmax += 1
                    if not (rho < 0 and qmax < p["max_trials"]):
                        break
                o["lm_iterations"][k] += 1
                if qmax == p["max_trials"] or rho == 0 or not np.isfinite(lam):
                    status = STALLED
                    break
                if converged:
                    status = CONVERGED
                    break
            o["status"][k], o["cost_final"][k] = status, 0.0 if status == FAILED else cur
            outlier, chi2 = self.classify(T, X)
            present = self.kind != 0
            o["inliers"][k] = int(np.sum(present & (outlier == 0)))
            m = np.abs(chi2[present] / self.d2[present] - 1.0)
            o["margins"].append(float(m[chi2[present] > 0].min()) if np.any(chi2[present] > 0) else 1.0)
            o["rounds_run"] = k + 1
            if status == FAILED:
                break
        o.update(poses=T, points=X, outlier=outlier, chi2=chi2)
        return o


def witness(g, **kw):
    """the round logic by the numpy witness: dict(poses, points, outlier, chi2, rounds_run, status, lm_iterations, inliers, cost_initial,
    cost_final per round, margins: per classification the smallest |chi2 / threshold - 1| over the present, defined edges)"""
    return Witness(g, **kw).run()
