"""ctypes loader of tests/popt_ref.c, the restatement of the stereo pose optimisation (ygz_slam_amd/csrc/popt.hip), a numpy witness of the same
spec written another way (vectorised residuals, the Jacobian by central differences through the retraction, np.linalg.solve for the 6 x 6 system,
np.sum for the sums), and the scenes that tests/test_popt_ref.py, tests/test_gpu_popt.py and tests/test_gpu_popt_surface.py share.  Test
infrastructure: compiled with gcc into a temporary directory the first time it is used, never imported by the package."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

FAILED, CONVERGED, MAX_ITERATIONS, STALLED = range(4)
TRIAL_REJECTED, TRIAL_ACCEPTED, TRIAL_FAILED, TRIAL_PIVOT = 0, 1, 2, 3
MAX_ROUNDS = 8
DMAX = 1.7976931348623157e308
# the context's default intrinsics (ygz_hip_default_params: config/default.yaml) as the floats it stores, converted to double
DEFAULT_K = tuple(float(np.float32(v)) for v in (520.9, 521.0, 325.1, 249.7))
WIDTH, HEIGHT, LEVELS, BASELINE = 640, 480, 4, 0.1
ROUND_OUTPUTS = ("status", "lm_iterations", "cost_initial", "cost_final", "lambda")
OUTPUTS = ("pose", "outlier", "chi2", "inliers", "rounds_run") + ROUND_OUTPUTS


class Params(ctypes.Structure):
    """pr_params = ygz_pose_opt_params"""
    _fields_ = [("baseline", ctypes.c_double), ("chi2_mono", ctypes.c_double), ("chi2_stereo", ctypes.c_double), ("rounds", ctypes.c_int32),
                ("iterations", ctypes.c_int32), ("max_trials", ctypes.c_int32), ("robust_rounds", ctypes.c_int32), ("min_edges", ctypes.c_int32),
                ("min_inliers", ctypes.c_int32), ("min_rel_decrease", ctypes.c_double)]


def params(**fields):
    """the scenes' parameters: the defaults of pr_default_params with the scenes' baseline and the relative-decrease stop switched on, then the
    given fields.  With min_rel_decrease = 0, g2o's rules iterate down to the rounding floor of the cost, where the sign of a gain ratio is decided
    by the last bit of a sum: the restatement and the device agree there bit for bit (tests/test_gpu_popt.py runs the plain defaults too), two
    programs that add in different orders cannot.  1e-6 ends every round CONVERGED four to five orders of magnitude above that floor."""
    p = Params()
    lib().pr_default_params(ctypes.byref(p))
    p.baseline, p.min_rel_decrease = BASELINE, 1e-6
    for k, v in fields.items():
        getattr(p, k)
        setattr(p, k, v)
    return p


def defaults(**fields):
    """pr_default_params alone (min_rel_decrease = 0) with the scenes' baseline, then the given fields"""
    return params(**dict(dict(min_rel_decrease=0.0), **fields))


def fields(p):
    return {n: getattr(p, n) for n, _ in Params._fields_}


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="popt_ref_")
        so = os.path.join(d, "libpopt_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "popt_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        i32, dbl, u8, pp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(Params)
        _lib.pr_default_params.argtypes = [pp]
        _lib.pr_default_params.restype = None
        _lib.pr_optimize.argtypes = [dbl, ctypes.c_int, dbl, dbl, i32, u8, pp, dbl, dbl, u8, dbl, i32, i32, i32, i32, dbl, dbl, dbl, i32, ctypes.c_int, i32]
        _lib.pr_optimize.restype = None
        _lib.pr_linearize.argtypes = [ctypes.c_int, dbl, dbl, i32, u8, dbl, dbl, ctypes.c_double, ctypes.c_double, dbl, dbl, dbl, i32, i32]
        _lib.pr_linearize.restype = None
        _lib.pr_jacobian.argtypes = [dbl, ctypes.c_int, dbl, dbl]
        _lib.pr_jacobian.restype = None
        _lib.pr_residual.argtypes = [dbl, dbl, dbl, dbl, ctypes.c_int, dbl, dbl, dbl]
        _lib.pr_rotation.argtypes = [dbl, dbl]
        _lib.pr_rotation.restype = None
        _lib.pr_retract.argtypes = [dbl, dbl, dbl]
        _lib.pr_retract.restype = None
        _lib.pr_project.argtypes = [dbl, dbl, dbl, dbl]
        _lib.pr_reduce.argtypes = [dbl]
        _lib.pr_reduce.restype = ctypes.c_double
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _d(a):
    return _p(a, ctypes.c_double)


def k5(baseline, K=DEFAULT_K):
    return np.array(list(K) + [K[0] * baseline])


class Frame:
    """the edges of one frame in the ABI's types, the entry pose, and what the scene knows about itself"""

    def __init__(self, X, obs, level, kind, pose, truth=None, is_outlier=None):
        self.X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        self.obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 3)
        self.level = np.ascontiguousarray(level, np.int32).reshape(-1)
        self.kind = np.ascontiguousarray(kind, np.uint8).reshape(-1)
        self.pose = np.ascontiguousarray(pose, np.float64).reshape(7)
        self.truth = None if truth is None else np.ascontiguousarray(truth, np.float64).reshape(7)
        self.is_outlier = None if is_outlier is None else np.asarray(is_outlier, bool)
        self.n = len(self.level)
        assert len(self.X) == len(self.obs) == len(self.kind) == self.n

    def replace(self, **kw):
        v = dict(X=self.X, obs=self.obs, level=self.level, kind=self.kind, pose=self.pose, truth=self.truth, is_outlier=self.is_outlier)
        v.update(kw)
        return Frame(**v)

    def compacted(self):
        keep = self.kind != 0
        return Frame(self.X[keep], self.obs[keep], self.level[keep], self.kind[keep], self.pose, self.truth,
                     None if self.is_outlier is None else self.is_outlier[keep])


def optimize(fr, p, K=DEFAULT_K):
    """pr_optimize on one frame: every output of the ABI for that frame plus `trace`, the (round, iteration, code) of every trial"""
    n, m = fr.n, max(fr.n, 1)
    pad = lambda a: a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)
    o = dict(pose=np.empty(7), outlier=np.zeros(m, np.uint8), chi2=np.zeros(m), inliers=np.zeros(1, np.int32), rounds_run=np.zeros(1, np.int32),
             status=np.zeros(MAX_ROUNDS, np.int32), lm_iterations=np.zeros(MAX_ROUNDS, np.int32), cost_initial=np.zeros(MAX_ROUNDS),
             cost_final=np.zeros(MAX_ROUNDS))
    o["lambda"] = np.zeros(MAX_ROUNDS)
    cap = max(1, p.rounds * p.iterations * p.max_trials)
    trace, nt = np.zeros(cap, np.int32), np.zeros(1, np.int32)
    Kd = np.array(K, np.float64)
    lib().pr_optimize(_d(Kd), n, _d(pad(fr.X)), _d(pad(fr.obs)), _p(pad(fr.level), ctypes.c_int32), _p(pad(fr.kind), ctypes.c_uint8), ctypes.byref(p),
                      _d(fr.pose), _d(o["pose"]), _p(o["outlier"], ctypes.c_uint8), _d(o["chi2"]), _p(o["inliers"], ctypes.c_int32),
                      _p(o["rounds_run"], ctypes.c_int32), _p(o["status"], ctypes.c_int32), _p(o["lm_iterations"], ctypes.c_int32),
                      _d(o["cost_initial"]), _d(o["cost_final"]), _d(o["lambda"]), _p(trace, ctypes.c_int32), cap, _p(nt, ctypes.c_int32))
    o["outlier"], o["chi2"] = o["outlier"][:n], o["chi2"][:n]
    o["inliers"], o["rounds_run"] = int(o["inliers"][0]), int(o["rounds_run"][0])
    assert nt[0] <= cap
    o["trace"] = [(int(c) >> 16, (int(c) >> 8) & 255, int(c) & 255) for c in trace[:nt[0]]]
    return o


def linearize(fr, T, p, robust=True, K=DEFAULT_K):
    """pr_linearize: H [21], b [6], cost, n_ok, n_rej of all edges with kind != 0 at T"""
    pad = lambda a: a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)
    H, b, cost, cnt = np.empty(21), np.empty(6), np.empty(1), np.zeros(2, np.int32)
    T = np.ascontiguousarray(T, np.float64)
    lib().pr_linearize(fr.n, _d(pad(fr.X)), _d(pad(fr.obs)), _p(pad(fr.level), ctypes.c_int32), _p(pad(fr.kind), ctypes.c_uint8), _d(k5(p.baseline, K)),
                       _d(T), p.chi2_mono if robust else 0.0, p.chi2_stereo if robust else 0.0, _d(H), _d(b), _d(cost),
                       _p(cnt, ctypes.c_int32), _p(cnt[1:], ctypes.c_int32))
    return dict(H=H, b=b, cost=float(cost[0]), n_ok=int(cnt[0]), n_rej=int(cnt[1]))


def jacobian(T, X, kind, baseline=BASELINE, K=DEFAULT_K):
    """pr_jacobian of one edge at T: [3, 6], or None when the edge is rejected"""
    T, X = np.ascontiguousarray(T, np.float64), np.ascontiguousarray(X, np.float64)
    R, P, r, J, K5 = np.empty(9), np.empty(3), np.empty(3), np.empty(18), k5(baseline, K)
    lib().pr_rotation(_d(T), _d(R))
    if not lib().pr_residual(_d(R), _d(T[4:].copy()), _d(X), _d(np.zeros(3)), int(kind), _d(K5), _d(P), _d(r)):
        return None
    lib().pr_jacobian(_d(P), int(kind), _d(K5), _d(J))
    return J.reshape(3, 6)


def project(T, X, baseline=BASELINE, K=DEFAULT_K):
    """pr_project of the points X [n, 3] at T: (u, v, uR) [n, 3] and the mask of the points in front of the camera"""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    T, K5 = np.ascontiguousarray(T, np.float64), k5(baseline, K)
    out, ok = np.zeros((len(X), 3)), np.zeros(len(X), bool)
    for i in range(len(X)):
        ok[i] = bool(lib().pr_project(_d(K5), _d(T), _d(X[i]), _d(out[i])))
    return out, ok


def retract(T, d):
    out = np.empty(7)
    lib().pr_retract(_d(np.ascontiguousarray(T, np.float64)), _d(np.ascontiguousarray(d, np.float64)), _d(out))
    return out


def reduce256(lane):
    return float(lib().pr_reduce(_d(np.ascontiguousarray(lane, np.float64))))


def uright_from_depth(u, depth, baseline, fx=DEFAULT_K[0]):
    """PoseOptimizer::URightFromDepth in numpy: u - bf / depth where depth > 0, -1 elsewhere"""
    u, depth = np.asarray(u, np.float64), np.asarray(depth, np.float64)
    safe = np.where(depth > 0, depth, 1.0)
    return np.where(depth > 0, u - (fx * baseline) / safe, -1.0)


# ---- the witness ------------------------------------------------------------------------------------------------------------------------
def w_rotation(q):
    x, y, z, w = q[:4]
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def w_qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def w_retract(T, d):
    dq = np.array([0.5 * d[0], 0.5 * d[1], 0.5 * d[2], 1.0])
    dq = dq / np.sqrt(np.sum(dq * dq))
    q = w_qmul(dq, T[:4])
    return np.concatenate([q / np.sqrt(np.sum(q * q)), w_rotation(dq) @ T[4:] + d[3:]])


def w_residuals(fr, T, K5):
    """all edges at once: r [n, 3] (column 2 zero for mono edges), accepted [n], chi2 [n].  The products are written in the restatement's
    association, so that a residual that is exactly zero there is exactly zero here (scene k)."""
    R, t = w_rotation(T), T[4:]
    X = fr.X
    P = [(R[i, 0] * X[:, 0] + R[i, 1] * X[:, 1] + R[i, 2] * X[:, 2]) + t[i] for i in range(3)]
    front = P[2] > 0
    z = np.where(front, P[2], 1.0)
    with np.errstate(all="ignore"):
        up = K5[0] * (P[0] / z) + K5[2]
        r = np.stack([fr.obs[:, 0] - up, fr.obs[:, 1] - (K5[1] * (P[1] / z) + K5[3]),
                      np.where(fr.kind == 2, fr.obs[:, 2] - (up - K5[4] / z), 0.0)], axis=1)
        ok = front & np.all(np.abs(r) <= DMAX, axis=1)
        w = 1.0 / 4.0 ** fr.level
        e2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        e2 = np.where(fr.kind == 2, e2 + r[:, 2] * r[:, 2], e2)
    r = np.where(ok[:, None], r, 0.0)
    return r, ok, np.where(ok, w * e2, 0.0), w


def w_robust(chi2, d2):
    """rho, rho' per edge; d2 [n] (<= 0: no kernel)"""
    big = (d2 > 0) & (chi2 > d2)
    s = np.sqrt(np.where(big, chi2, 1.0))
    delta = np.sqrt(np.where(d2 > 0, d2, 1.0))
    return np.where(big, 2.0 * s * delta - d2, chi2), np.where(big, delta / s, 1.0)


W_STEP = 1e-6


def w_jacobians(fr, T, K5):
    """dr/d(omega, t) [n, 3, 6] by central differences through the retraction"""
    J = np.zeros((fr.n, 3, 6))
    # the translation step follows the scene's depths where they are below a metre (1e-6 for every ordinary scene)
    z = np.abs((fr.X @ w_rotation(T).T + T[4:])[:, 2]) if fr.n else np.ones(1)
    steps = [W_STEP] * 3 + [W_STEP * min(1.0, float(np.median(z)))] * 3
    for k in range(6):
        d = np.zeros(6)
        d[k] = steps[k]
        rp = w_residuals(fr, w_retract(T, d), K5)[0]
        rm = w_residuals(fr, w_retract(T, -d), K5)[0]
        with np.errstate(all="ignore"):
            J[:, :, k] = (rp - rm) / (2.0 * steps[k])
    return J


def w_pass(fr, T, K5, active, d2, full):
    r, ok, chi2, w = w_residuals(fr, T, K5)
    use = active & ok
    rho, rho1 = w_robust(chi2, d2)
    out = dict(cost=float(np.sum(rho[use])), n_ok=int(use.sum()), n_rej=int((active & ~ok).sum()))
    if full:
        J = w_jacobians(fr, T, K5)[use]
        ww = (rho1 * w)[use]
        out["H"] = np.einsum("e,eia,eib->ab", ww, J, J)
        out["b"] = -np.einsum("e,eia,ei->a", ww, J, r[use])
    return out


def witness(fr, p, K=DEFAULT_K):
    """the spec in numpy: the outputs of optimize()"""
    K5 = k5(p.baseline, K)
    n = fr.n
    outlier, chi2 = np.zeros(n, np.uint8), np.zeros(n)
    o = dict(status=np.zeros(MAX_ROUNDS, np.int32), lm_iterations=np.zeros(MAX_ROUNDS, np.int32), cost_initial=np.zeros(MAX_ROUNDS),
             cost_final=np.zeros(MAX_ROUNDS), trace=[])
    o["lambda"] = np.zeros(MAX_ROUNDS)
    finite = lambda v: abs(v) <= DMAX
    T, inl, run = fr.pose.copy(), 0, 0
    for k in range(p.rounds):
        T = fr.pose.copy()
        active = (fr.kind != 0) & (outlier == 0)
        robust = k < p.robust_rounds
        d2 = np.where(fr.kind == 2, p.chi2_stereo, p.chi2_mono) if robust else np.zeros(n)
        lam, ni, chi, st, iters = 0.0, 2.0, 0.0, MAX_ITERATIONS, 0
        for it in range(p.iterations):
            L = w_pass(fr, T, K5, active, d2, True)
            if it == 0:
                if L["n_ok"] < p.min_edges or not finite(L["cost"]):
                    st = FAILED
                    break
                o["cost_initial"][k] = L["cost"]
                lam, ni = 1e-5 * float(np.max(np.abs(np.diag(L["H"])))), 2.0
            chi = L["cost"]
            rho, qmax, converged = 0.0, 0, False
            while True:
                temp, scale, ok = DMAX, 0.0, True
                with np.errstate(all="ignore"):
                    A = L["H"] + np.diag(np.full(6, lam))
                    try:                                                   # positive definite and finite, as the restatement's pivots
                        ok = bool(np.isfinite(A).all())
                        if ok:
                            C6 = np.linalg.cholesky(A)
                            ok = bool(np.isfinite(C6).all() and np.isfinite(np.diag(C6) ** 2).all())
                        if ok:
                            d = np.linalg.solve(C6.T, np.linalg.solve(C6, L["b"]))
                    except np.linalg.LinAlgError:
                        ok = False
                solved = ok
                if ok:
                    scale = float(np.sum(d * (lam * d + L["b"])))
                    Tn = T.copy() if not d.any() else w_retract(T, d)
                    C = w_pass(fr, Tn, K5, active, d2, False)
                    temp = C["cost"]
                    ok = C["n_rej"] <= L["n_rej"] and finite(temp)
                    if not ok:
                        temp, scale = DMAX, 0.0
                scale += 1e-3
                with np.errstate(all="ignore"):
                    rho = float((np.float64(chi) - np.float64(temp)) / np.float64(scale))
                if not finite(rho):
                    rho = -1.0
                accepted = ok and rho > 0
                o["trace"].append((k, it, TRIAL_ACCEPTED if accepted else TRIAL_REJECTED if ok else TRIAL_FAILED if solved else TRIAL_PIVOT))
                stop = False
                if accepted:
                    lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
                    ni = 2.0
                    converged = chi - temp <= p.min_rel_decrease * chi
                    chi, T = temp, Tn
                else:
                    with np.errstate(all="ignore"):
                        lam, ni = float(np.float64(lam) * ni), ni * 2.0
                    stop = not finite(lam)
                if not stop:
                    qmax += 1
                if stop or not (rho < 0 and qmax < p.max_trials):
                    break
            iters += 1
            if qmax == p.max_trials or rho == 0 or not finite(lam):
                st = STALLED
                break
            if converged:
                st = CONVERGED
                break
        o["status"][k], o["lm_iterations"][k], o["lambda"][k] = st, iters, lam
        o["cost_final"][k] = 0.0 if st == FAILED else chi
        r, ok, c, w = w_residuals(fr, T, K5)
        th = np.where(fr.kind == 2, p.chi2_stereo, p.chi2_mono)
        present = fr.kind != 0
        chi2 = np.where(present, c, -1.0)
        outlier = (present & (~ok | (c > th))).astype(np.uint8)
        inl, run = int((present & (outlier == 0)).sum()), k + 1
        if inl < p.min_inliers:
            break
    o.update(pose=T, outlier=outlier, chi2=chi2, inliers=inl, rounds_run=run)
    return o


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------
def _quat(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([axis * np.sin(angle / 2), [np.cos(angle / 2)]])


def make_frame(seed, n, kinds="alternate", outliers=0.0, noise=True, perturb=True, behind=False, K=DEFAULT_K, n_outliers=None, coherent=False):
    """n points at depths 2 .. 20 m in front of a ground-truth pose, seen with Gaussian noise of 0.5 * 2^level pixels (uR too); levels cycle
    0 .. 3; gross outliers are displaced by 20 .. 60 pixels (times the level's scale, so that their chi2 is >= 25 at every level); the entry pose
    is the truth perturbed by 2 degrees and 5 cm"""
    # (the displacements are in pixels of the edge's level: 20 level-0 pixels at level 3 would be a chi2 of 6.25, next to the threshold)
    rng = np.random.RandomState(seed)
    truth = np.concatenate([_quat(rng.randn(3), 0.3 * rng.rand()), 0.5 * rng.randn(3)])
    level = (np.arange(n) % LEVELS).astype(np.int32)
    z = rng.uniform(2.0, 20.0, n)
    u, v = rng.uniform(40, WIDTH - 40, n), rng.uniform(40, HEIGHT - 40, n)
    Pc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    if behind:
        Pc[:, 2] = -Pc[:, 2]
    R, t = w_rotation(truth), truth[4:]
    X = (Pc - t) @ R                                                   # R^T (Pc - t)
    if behind:
        obs = np.stack([u, v, u - K[0] * BASELINE / z], axis=1)
    else:
        obs, ok = project(truth, X, K=K)
        assert ok.all()
    scale = 2.0 ** level
    if noise:
        obs = obs + 0.5 * scale[:, None] * rng.randn(n, 3)
    n_out = int(round(outliers * n)) if n_outliers is None else n_outliers
    is_out = np.zeros(n, bool)
    if n_out:
        is_out[rng.permutation(n)[:n_out]] = True
        ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(20.0, 60.0, n) * scale
        if coherent:                                                      # all displaced roughly one way: they pull the first round's pose
            ang = rng.uniform(0, 2 * np.pi) + rng.uniform(-0.3, 0.3, n)
        obs[is_out, 0] += (mag * np.cos(ang))[is_out]
        obs[is_out, 1] += (mag * np.sin(ang))[is_out]
        obs[is_out, 2] += (mag * np.cos(ang))[is_out] + (rng.uniform(20.0, 60.0, n) * scale * rng.choice([-1.0, 1.0], n))[is_out]
    if kinds == "stereo":
        kind = np.full(n, 2, np.uint8)
    elif kinds == "mono":
        kind = np.full(n, 1, np.uint8)
    else:
        kind = (1 + np.arange(n) % 2).astype(np.uint8)
    pose = truth.copy()
    if perturb:
        deg, metres = (2.0, 0.05) if perturb is True else perturb
        d = np.concatenate([np.deg2rad(deg) * _unit(rng), metres * _unit(rng)])
        pose = w_retract(truth, d)
    return Frame(X, obs, level, kind, pose, truth, is_out)


def tiny_frame(n, z, offset):
    """n mono edges of level 0 on the optical axis at the depths z, seen `offset` pixels from the principal point, at the identity pose"""
    X = np.stack([np.zeros(n), np.zeros(n), np.asarray(z, np.float64)], axis=1)
    obs = np.concatenate([np.array(DEFAULT_K[2:4]) + offset, np.zeros((n, 1))], axis=1)
    return Frame(X, obs, np.zeros(n, np.int32), np.ones(n, np.uint8), [0, 0, 0, 1, 0, 0, 0.0])


def _unit(rng):
    v = rng.randn(3)
    return v / np.linalg.norm(v)


J_SIZES = (1, 3, 63, 64, 65, 255, 256, 257)
SCENES = ("a", "b", "c", "d", "e", "f", "g", "h", "i", "j", "k", "l0", "l4", "l1r", "l1i", "m", "n", "o", "p", "q", "r")
# the seed of every scene; a scene with an edge within 1 % of its threshold at the restatement's final pose is reseeded (tests/test_popt_ref.py
# checks the margin)
SEEDS = dict(a=101, b=102, c=103, d=104, e=201, f=106, g=107, h=103, i=109, j=110, k=111, l=103, n=407, o=115, q=2003)
_scenes = {}


def scene(name):
    """(frames, params) of a scene; frames is a list (one frame except for j).  Built once and shared: do not modify."""
    if name not in _scenes:
        _scenes[name] = _build(name)
    return _scenes[name]


def _build(name):
    p = params()
    if name == "a":
        return [make_frame(SEEDS["a"], 300, "stereo")], p
    if name == "b":
        return [make_frame(SEEDS["b"], 300, "mono")], p
    if name == "c":
        return [make_frame(SEEDS["c"], 300, outliers=0.15)], p
    if name == "d":
        return [make_frame(SEEDS["d"], 300, outliers=0.40, coherent=True)], p
    if name == "e":
        return [make_frame(SEEDS["e"], 42, n_outliers=30)], p
    if name == "f":
        return [make_frame(SEEDS["f"], 2)], p
    if name == "g":
        return [make_frame(SEEDS["g"], 300, behind=True)], p
    if name == "h":
        fr = make_frame(SEEDS["h"], 300, outliers=0.15)
        kind = fr.kind.copy()
        kind[np.random.RandomState(7).permutation(300)[:100]] = 0
        return [fr.replace(kind=kind)], p
    if name == "i":
        return [make_frame(SEEDS["i"], 1100, outliers=0.15)], p
    if name == "j":
        return [make_frame(SEEDS["j"] + q, n, outliers=0.15) for q, n in enumerate(J_SIZES)], p
    if name == "k":
        return [make_frame(SEEDS["k"], 300, noise=False, perturb=False)], p
    fr = make_frame(SEEDS["l"], 300, outliers=0.15)
    if name == "l0":
        return [fr], params(robust_rounds=0)
    if name == "l4":
        return [fr], params(robust_rounds=4)
    if name == "l1r":
        return [fr], params(rounds=1)
    if name == "l1i":
        return [fr], params(iterations=1)
    if name == "m":                                                        # one trial per iteration: STALLED by the trial count
        return [fr], params(max_trials=1)
    if name == "n":    # a wild entry pose (90 degrees, 6 m) and no kernel: trials are rejected, and some fail on points behind the trial pose
        return [make_frame(SEEDS["n"], 300, outliers=0.15, perturb=(90.0, 6.0))], params(robust_rounds=0)
    if name == "o":    # (c) with every 17th point behind the entry pose: rejected in every evaluation, counted, and the rounds still run
        fr = make_frame(SEEDS["o"], 300, outliers=0.15)
        R, t = w_rotation(fr.truth), fr.truth[4:]
        Pc = fr.X @ R.T + t
        Pc[::17, 2] = -Pc[::17, 2]
        return [fr.replace(X=(Pc - t) @ R)], p
    if name == "p":    # five mono edges a hair in front of the camera: (fx / z)^2 overflows while the cost is 10, so lambda_0 is infinite
        return [tiny_frame(5, np.full(5, 1e-160), np.ones((5, 2)))], p
    if name == "q":    # depths near 1e-151: H stays finite, lambda grows through rejected trials until H + lambda I overflows, the pivot fails
        rng = np.random.RandomState(SEEDS["q"])    # with a finite lambda, trial after trial without a pass, and lambda itself overflows
        z = 10.0 ** rng.uniform(-151.2, -150.8) * rng.uniform(0.5, 1.5, 4)
        return [tiny_frame(4, z, 100.0 * rng.randn(4, 2))], params(max_trials=64, robust_rounds=0)
    if name == "r":    # no edge at all and min_edges = 0: H = 0, lambda_0 = 0, every pivot fails, STALLED by the trial count
        fr = make_frame(SEEDS["c"], 300, outliers=0.15)
        return [fr.replace(kind=np.zeros(300, np.uint8))], params(min_edges=0)
    raise KeyError(name)


def mixed_call(n_frames=64):
    """n_frames frames of mixed scenes for one call with the default parameters: the single-frame scenes a .. k and the frames of j, repeated"""
    pool = []
    for name in ("a", "b", "c", "d", "e", "f", "g", "h", "j", "k"):
        pool += scene(name)[0]
    return [pool[q % len(pool)] for q in range(n_frames)]


def pack(frames):
    """the CSR arrays of the ABI for a list of frames"""
    off = np.zeros(len(frames) + 1, np.int32)
    off[1:] = np.cumsum([f.n for f in frames])
    cat = lambda key, shape, dt: (np.concatenate([getattr(f, key) for f in frames]) if frames else np.zeros(shape, dt))
    return dict(frame_off=off, pw=cat("X", (0, 3), np.float64), obs=cat("obs", (0, 3), np.float64), level=cat("level", 0, np.int32),
                kind=cat("kind", 0, np.uint8), poses=np.stack([f.pose for f in frames]) if frames else np.zeros((0, 7)))
