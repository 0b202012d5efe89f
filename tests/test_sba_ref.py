"""CPU tests of tests/sba_ref.c, the frozen restatement of the stereo bundle adjustment, against its witnesses: (a) the
global bundle adjustment's restatement, bit for bit, on mono level-0 kernel-free problems; (b) every Jacobian row against central
differences; (c) the final cost of a stereo scene against scipy's Levenberg-Marquardt; (d) the round logic against the numpy witness of
tests/sba_ref.py; (e) the scale of a scene started 5 % too large, which mono edges cannot see and stereo edges recover; (f) the branches of
the rounds, by name."""
import numpy as np
import pytest

import gba_ref as gb
import sba_cases as sc
import sba_ref as sb
from test_gpu_gba import SHAPES


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def answers():
    """the restatement's answers to the scenes of (d) and (f), computed once"""
    out = {}
    for group in (sc.SCENES_D, sc.SCENES_F):
        for name, (make, kw) in group.items():
            g = make()
            out[name] = (g, kw, sb.optimize(g, **kw))
    return out


# ---- (a) the old solver -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_mono_level0_without_kernel_is_the_global_bundle_adjustment(name):
    """every shape of tests/test_gpu_gba.py with its Huber kernel switched off, as mono edges of level 0, robust_rounds 0, one round of the
    shape's iterations (10 unless the shape says otherwise): poses, points, costs, lambda, status and all counters carry the bits of
    gba_ref.optimize, and the stage export those of gba_ref.linearize on the shared columns"""
    make, kw = SHAPES[name]
    g = dict(make(), huber=0.0)
    kw = dict(kw)
    old = gb.optimize(g, **kw)
    it = kw.pop("max_iterations", 10)
    s = sb.as_gba(g)
    new = sb.optimize(s, rounds=1, robust_rounds=0, iterations=(it,), **kw)
    assert new["rounds_run"] == 1
    for a, b in [("status", "status"), ("lm_iterations", "lm_iterations"), ("n_solves", "n_solves"), ("cg_iterations_total", "cg_iterations"),
                 ("cg_capped", "cg_capped")]:
        assert old[a] == new[b][0], (a, old[a], new[b][0])
    for a in ("cost_initial", "cost_final", "lambda_"):
        assert _bits([old[a]])[0] == _bits([new[a][0]])[0], (a, old[a], new[a][0])
    assert np.array_equal(_bits(old["poses"]), _bits(new["poses"])) and np.array_equal(_bits(old["points"]), _bits(new["points"]))
    assert old["status"] != gb.FAILED and np.all(new["chi2"] >= 0)
    lo, ln = gb.linearize(g), sb.linearize(s, robust_rounds=0)
    assert lo["ok"] and ln["ok"] and _bits([lo["cost"]])[0] == _bits([ln["cost"]])[0]
    for k in ("w", "Hpp", "bp", "Hll", "bl"):
        assert np.array_equal(_bits(lo[k]), _bits(ln[k])), k
    for k in ("res", "Jp", "Jl"):
        assert np.array_equal(_bits(lo[k]), _bits(ln[k][:, :2])), k
        assert np.all(ln[k][:, 2] == 0.0)


# ---- (b) Jacobians ------------------------------------------------------------------------------------------------------------------------
def test_jacobian_rows_against_central_differences():
    """80 random mono and stereo edges at depths of 2 to 6 m, every level, residuals of some pixels, then every edge of the (d) scene
    half_8x80_outliers at its start: all three rows of both blocks against central differences (h = 1e-6) through the restatement's own
    retraction for the pose and an additive step for the point.  Largest
    deviation measured: 6.34e-8 (JACOBIAN_MEASURED); asserted at 10 x that"""
    rng = np.random.default_rng(3)
    h, worst = 1e-6, 0.0
    for i in range(80):
        kind, level = 1 + i % 2, (i // 2) % 4
        T = gb.look_at(rng.uniform(-1, 1, 3) + [0, 0, -4], rng.uniform(-0.3, 0.3, 3))
        X = rng.uniform(-1, 1, 3)
        px, z = gb.project(T, X)
        ob = np.array([px[0], px[1], px[0] - sb.K4[0] * sb.BASELINE / z]) + rng.normal(0, 3, 3)
        ok, r, w, rho, Jp, Jl = sb.edge_terms(T, X, ob, kind, level)
        assert ok and w == 0.25 ** level and (kind == 2 or (r[2] == 0.0 and np.all(Jp[2] == 0.0) and np.all(Jl[2] == 0.0)))
        assert kind == 1 or (r[2] != 0.0 and np.all(Jl[2] != 0.0))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            rp, rm = sb.edge_terms(gb.retract(T, d), X, ob, kind, level)[1], sb.edge_terms(gb.retract(T, -d), X, ob, kind, level)[1]
            worst = max(worst, np.abs((rp - rm) / (2 * h) - Jp[:, k]).max())
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            rp, rm = sb.edge_terms(T, X + d, ob, kind, level)[1], sb.edge_terms(T, X - d, ob, kind, level)[1]
            worst = max(worst, np.abs((rp - rm) / (2 * h) - Jl[:, k]).max())
    # every edge of a (d) scene at its start: 320 edges, half of them stereo, levels 0 to 3, a tenth displaced
    g = sc.SCENES_D["half_8x80_outliers"][0]()
    bf = g["K"][0] * g["baseline"]
    for e in range(len(g["obs"])):
        T, X, ob, kind, level = g["poses"][g["edge_pose"][e]], g["points"][g["edge_point"][e]], g["obs"][e], int(g["kind"][e]), int(g["level"][e])
        ok, r, w, rho, Jp, Jl = sb.edge_terms(T, X, ob, kind, level, g["K"], bf)
        assert ok
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            rp, rm = sb.edge_terms(gb.retract(T, d), X, ob, kind, level, g["K"], bf)[1], sb.edge_terms(gb.retract(T, -d), X, ob, kind, level, g["K"], bf)[1]
            worst = max(worst, np.abs((rp - rm) / (2 * h) - Jp[:, k]).max())
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            rp, rm = sb.edge_terms(T, X + d, ob, kind, level, g["K"], bf)[1], sb.edge_terms(T, X - d, ob, kind, level, g["K"], bf)[1]
            worst = max(worst, np.abs((rp - rm) / (2 * h) - Jl[:, k]).max())
    print("largest difference from central differences: %.3g" % worst)
    assert worst <= 10 * JACOBIAN_MEASURED


JACOBIAN_MEASURED = 6.34e-8


# ---- (c) scipy ------------------------------------------------------------------------------------------------------------------------------
def _scipy_cost(g):
    from scipy.optimize import least_squares
    T0, fixed, X0, ep, el, obs, kind, level = sb.arrays(g)
    free = np.flatnonzero(fixed == 0)
    K, bf, sw = g["K"], g["K"][0] * g["baseline"], np.sqrt(0.25 ** level.astype(float))

    def fun(x):
        T = T0.copy()
        for k, v in enumerate(free):
            T[v] = gb.retract(T0[v], x[6 * k:6 * k + 6])
        X = X0 + x[6 * len(free):].reshape(-1, 3)
        R = np.array([gb.rotation(t[:4]) for t in T])
        P = np.einsum("eij,ej->ei", R[ep], X[el]) + T[ep, 4:]
        u = K[0] * P[:, 0] / P[:, 2] + K[2]
        r = np.stack([obs[:, 0] - u, obs[:, 1] - (K[1] * P[:, 1] / P[:, 2] + K[3]), np.where(kind == 2, obs[:, 2] - (u - bf / P[:, 2]), 0.0)], axis=1)
        return (sw[:, None] * r).ravel()
    sol = least_squares(fun, np.zeros(6 * len(free) + 3 * len(X0)), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=100000)
    return 2.0 * sol.cost


def test_final_cost_against_scipy_without_the_kernel():
    """5 poses x 40 points, half the edges stereo, levels 0 to 3, no outliers, no kernel, one round of up to 50 iterations: the final cost
    against scipy.optimize.least_squares(method="lm") on the same weighted residuals.  Measured relative difference 4.75e-11
    (SCIPY_MEASURED); asserted at 10 x that, 4.75e-10, which is below section 15's 1e-9"""
    g = sb.scene(5, 40, 3, seed=21)
    out = sb.optimize(g, rounds=1, robust_rounds=0, iterations=(50,))
    ref = _scipy_cost(g)
    rel = abs(out["cost_final"][0] - ref) / ref
    print("cost %.17g -> %.17g, scipy %.17g, relative difference %.3g, status %d, %d LM iterations"
          % (out["cost_initial"][0], out["cost_final"][0], ref, rel, out["status"][0], out["lm_iterations"][0]))
    assert out["status"][0] == sb.CONVERGED and out["cost_final"][0] < out["cost_initial"][0]
    assert rel <= 10 * SCIPY_MEASURED


SCIPY_MEASURED = 4.75e-11


# ---- (d) the numpy witness ------------------------------------------------------------------------------------------------------------------
WITNESS_MEASURED = 3.18e-9


@pytest.mark.parametrize("name", list(sc.SCENES_D))
def test_round_logic_against_the_numpy_witness(answers, name):
    """equal outlier flags, inlier counts, rounds_run, round statuses and LM iteration counts; at every classification no chi2 within 1 % of its threshold (or a
    witness that sums in another order could not be held to equal flags); poses and points within 10 x the largest deviation measured over
    the scenes, 3.18e-9 (half_8x80_outliers; WITNESS_MEASURED)"""
    g, kw, ref = answers[name]
    wit = sb.witness(g, **kw)
    print("%s: rounds %d / %d, status %s / %s, LM iterations %s / %s, inliers %s / %s, margins %s" % (
        name, ref["rounds_run"], wit["rounds_run"], ref["status"], wit["status"], ref["lm_iterations"], wit["lm_iterations"], ref["inliers"],
        wit["inliers"], wit["margins"]))
    assert min(wit["margins"]) > 0.01
    assert ref["rounds_run"] == wit["rounds_run"] == 2
    assert np.array_equal(ref["status"], wit["status"]) and np.array_equal(ref["inliers"], wit["inliers"])
    assert np.array_equal(ref["lm_iterations"], wit["lm_iterations"])
    assert np.array_equal(ref["outlier"], wit["outlier"])
    present = g["kind"] != 0
    m = np.abs(ref["chi2"][present] / np.where(g["kind"][present] == 2, sb.CHI2_STEREO, sb.CHI2_MONO) - 1.0)
    assert m.min() > 0.01
    dev = max(np.abs(ref["poses"] - wit["poses"]).max(), np.abs(ref["points"] - wit["points"]).max())
    print("largest deviation of a pose or point entry: %.3g" % dev)
    assert dev <= 10 * WITNESS_MEASURED
    if "outliers" in name:
        assert ref["outlier"][g["displaced"]].mean() > 0.9 and 0 < ref["outlier"].sum() < 0.3 * len(ref["outlier"])


# ---- (e) scale --------------------------------------------------------------------------------------------------------------------------------
def _scaled_start(stereo, s=1.05):
    """8 poses x 80 points seen four times, noise of 0.5 x 2^level pixels, one fixed camera; the start is the truth scaled by s about that camera's
    centre, the translations of the poses and the points alike"""
    g = sb.scene(8, 80, 4, stereo=stereo, seed=61, perturb=(0.0, 0.0, 0.0))
    R0 = gb.rotation(g["truth_poses"][0][:4])
    C0 = -R0.T @ g["truth_poses"][0][4:]
    g["points"] = C0 + s * (g["truth_points"] - C0)
    for v in range(len(g["poses"])):
        R = gb.rotation(g["truth_poses"][v][:4])
        C = -R.T @ g["truth_poses"][v][4:]
        g["poses"][v][4:] = -R @ (C0 + s * (C - C0))
    return g, C0


def _scale_error(points, g, C0):
    return abs(np.linalg.norm(points - C0, axis=1).sum() / np.linalg.norm(g["truth_points"] - C0, axis=1).sum() - 1.0)


SCALE_MEASURED = 1.22e-3


def test_stereo_edges_recover_the_scale_that_mono_edges_cannot_see():
    """why the feature exists.  The mono cost is exactly invariant under a scaling about the fixed camera, so a map started 5 % too large
    stays more than 4 % too large (measured 5.009 %); the same edges with their uR columns bring it back to the noise: measured
    1.22e-3 (SCALE_MEASURED), asserted at 10 x that"""
    g, C0 = _scaled_start("none")
    assert abs(_scale_error(g["points"], g, C0) - 0.05) < 1e-12
    mono = sb.optimize(g)
    e_mono = _scale_error(mono["points"], g, C0)
    g, C0 = _scaled_start("all")
    st = sb.optimize(g)
    e_st = _scale_error(st["points"], g, C0)
    print("scale error 0.05 -> mono %.6g (cost %.3g -> %.3g), stereo %.3g (cost %.6g -> %.3g)"
          % (e_mono, mono["cost_initial"][0], mono["cost_final"][mono["rounds_run"] - 1], e_st, st["cost_initial"][0], st["cost_final"][st["rounds_run"] - 1]))
    assert mono["status"][0] != sb.FAILED and st["status"][0] != sb.FAILED
    assert e_mono > 0.04
    assert e_st <= 10 * SCALE_MEASURED


# ---- (f) the branches -------------------------------------------------------------------------------------------------------------------------
def _after_round_0(g, kw):
    kw = dict(kw, rounds=1, robust_rounds=min(kw.get("robust_rounds", 1), 1), iterations=tuple(kw.get("iterations", (5,)))[:1])
    return sb.optimize(g, **kw)


def test_two_rounds_with_flags_that_change_between_them(answers):
    g, kw, out = answers["flags_change_between_rounds"]
    first = _after_round_0(g, kw)
    assert out["rounds_run"] == 2 and out["inliers"][0] == first["inliers"][0]
    assert not np.array_equal(first["outlier"], out["outlier"]) and out["inliers"][1] != out["inliers"][0]
    assert out["cost_initial"][1] < out["cost_final"][0]              # round 1 starts without the outliers and without the kernel


def test_failed_in_round_0_returns_the_input(answers):
    g, kw, out = answers["failed_in_round_0"]
    assert out["rounds_run"] == 1 and out["status"][0] == sb.FAILED and out["lm_iterations"][0] == 0 and out["cost_final"][0] == 0.0
    assert np.array_equal(_bits(out["poses"]), _bits(g["poses"])) and np.array_equal(_bits(out["points"]), _bits(g["points"]))
    behind = np.flatnonzero((out["outlier"] == 1) & (out["chi2"] == 0.0))
    assert len(behind) >= 1 and set(g["edge_point"][behind]) == {5}
    assert not sb.linearize(g)["ok"]
    assert out["inliers"][0] == int((out["outlier"] == 0).sum())


def _active_after_round_0(g, kw):
    first = _after_round_0(g, kw)
    return (g["kind"] != 0) & (first["outlier"] == 0)


def test_point_left_with_one_active_edge(answers):
    g, kw, out = answers["point_left_with_one_active_edge"]
    deg = np.bincount(g["edge_point"][_active_after_round_0(g, kw)], minlength=len(g["points"]))
    assert (deg == 1).any()
    assert out["rounds_run"] == 2 and out["status"][1] not in (sb.FAILED, sb.STALLED) and out["cost_final"][1] < out["cost_initial"][1]
    assert np.isfinite(out["points"]).all()


def test_free_pose_left_without_an_active_edge(answers):
    g, kw, out = answers["free_pose_left_without_an_edge"]
    deg = np.bincount(g["edge_pose"][_active_after_round_0(g, kw)], minlength=len(g["poses"]))
    assert deg[3] == 0 and g["fixed"][3] == 0
    first = _after_round_0(g, kw)
    assert np.array_equal(_bits(out["poses"][3]), _bits(first["poses"][3]))          # an empty block's step is zero
    assert out["rounds_run"] == 2 and out["status"][1] not in (sb.FAILED, sb.STALLED)


def test_round_with_no_active_edge_stalls(answers):
    g, kw, out = answers["round_with_no_active_edge"]
    first = _after_round_0(g, kw)
    assert first["inliers"][0] == 0 and first["outlier"].all()
    assert out["rounds_run"] == 2 and out["status"][1] == sb.STALLED and out["lambda_"][1] == 0.0 and out["n_solves"][1] == 0
    assert out["lm_iterations"][1] == 1 and out["cost_initial"][1] == 0.0 and out["cost_final"][1] == 0.0
    assert np.array_equal(_bits(out["poses"]), _bits(first["poses"])) and np.array_equal(_bits(out["points"]), _bits(first["points"]))


def test_kind_0_entries_among_the_edges(answers):
    g, kw, out = answers["kind_0_among_the_edges"]
    absent = g["kind"] == 0
    assert absent.sum() == 64 and np.all(out["chi2"][absent] == -1.0) and np.all(out["outlier"][absent] == 0)
    assert np.all(out["chi2"][~absent] >= 0) and out["inliers"][1] == int((out["outlier"][~absent] == 0).sum())
    lin = sb.linearize(g)
    assert lin["ok"] and np.all(lin["res"][absent] == 0.0) and np.all(lin["w"][absent] == 0.0) and np.all(lin["Jp"][absent] == 0.0)
    assert np.all(lin["Jl"][absent] == 0.0) and np.isfinite(lin["cost"])


def test_repeated_edge_counts(answers):
    g, kw, out = answers["repeated_edge"]
    a = sb.scene(4, 30, 3, seed=25)
    la, lb = sb.linearize(a), sb.linearize(g)
    assert len(lb["res"]) == len(la["res"]) + 1 and lb["cost"] > la["cost"]
    assert not np.array_equal(sb.optimize(a, **kw)["points"][0], out["points"][0])


def test_two_fixed_poses_keep_their_bits(answers):
    g, kw, out = answers["two_fixed_poses"]
    for v in range(6):
        assert np.array_equal(_bits(out["poses"][v]), _bits(g["poses"][v])) == (v in (1, 4)), v


def test_rounds_1_and_4(answers):
    one, four = answers["rounds_1"][2], answers["rounds_4"][2]
    assert one["rounds_run"] == 1 and one["lm_iterations"][0] == 7 and np.all(one["status"][1:] == 0) and np.all(one["inliers"][1:] == 0)
    assert four["rounds_run"] == 4 and list(four["lm_iterations"]) == [3, 4, 5, 6] and np.all(four["status"] == sb.MAX_ITERATIONS)


def test_robust_rounds_0_and_4(answers):
    g, _, none = answers["robust_rounds_0"]
    _, _, all4 = answers["robust_rounds_4"]
    lin0, lin1 = sb.linearize(g, robust_rounds=0), sb.linearize(g, robust_rounds=4)
    assert np.array_equal(lin0["w"], 0.25 ** g["level"].astype(float)) and (lin1["w"] < lin0["w"]).sum() >= g["displaced"].sum()
    assert none["cost_initial"][0] == lin0["cost"] and all4["cost_initial"][0] == lin1["cost"] and lin1["cost"] < lin0["cost"]
    assert all4["rounds_run"] == 4 and all4["cost_initial"][3] > 0


def test_rejected_trial(answers):
    out = answers["rejected_trial"][2]
    assert out["n_solves"][0] > out["lm_iterations"][0] and out["status"][0] == sb.STALLED


def test_capped_cg(answers):
    out = answers["capped_cg"][2]
    assert out["cg_capped"][0] >= 1 and out["cg_iterations"][0] <= 3 * out["n_solves"][0]
    assert out["cost_final"][0] < out["cost_initial"][0]
