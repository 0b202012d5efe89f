"""CPU tests of tests/pgo_ref.c, the frozen restatement of the Sim3 pose-graph optimiser: the algebra, the exact
Jacobians against central differences, the final cost against scipy's Levenberg-Marquardt on the same residual (the witness), convergence to
the truth on consistent graphs, and the rules that make the undefined cases definite (fix_scale, zero-residual components, fixed vertices,
a CG cap)."""
import numpy as np
import pytest

import pgo_ref as pg


def _random_sim3(rng, deg=40.0, t=2.0, ls=0.3):
    return pg.sim3(rng.normal(size=3), rng.uniform(0, deg), rng.uniform(-t, t, 3), np.exp(rng.uniform(-ls, ls)))


def test_lift_inverts_delta():
    rng = np.random.default_rng(1)
    for _ in range(50):
        x = np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-3, 3, 3), rng.uniform(-1.5, 1.5, 1)])
        ok, r = pg.lift(pg.delta(x))
        assert ok and np.abs(r - x).max() <= 1e-12
    ok, _ = pg.retract(pg.IDENTITY, [0, 0, 0, 0, 0, 0, 2.0])
    assert not ok                                                   # |sigma| >= 2 is rejected
    ok, _ = pg.lift([1.0, 0, 0, 0.0, 0, 0, 0, 1])
    assert not ok                                                   # a rotation of 180 degrees
    ok, _ = pg.lift([0, 0, 0, 1, np.inf, 0, 0, 1])
    assert not ok


def test_compose_and_inverse_agree_with_matrices():
    rng = np.random.default_rng(2)

    def mat(S):
        x, y, z, w = S[:4]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        T = np.eye(4)
        T[:3, :3] = S[7] * R
        T[:3, 3] = S[4:7]
        return T
    for _ in range(20):
        A, B = _random_sim3(rng), _random_sim3(rng)
        assert np.abs(mat(pg.compose(A, B)) - mat(A) @ mat(B)).max() < 1e-12
        assert np.abs(mat(pg.inverse(A)) @ mat(A) - np.eye(4)).max() < 1e-12


@pytest.mark.parametrize("fix_scale", [False, True])
def test_jacobians_against_central_differences(fix_scale):
    """random edges whose error reaches 10 degrees, 0.5 m and a scale of e^+-0.2: both blocks within 1e-6 of central differences, h = 1e-6"""
    rng = np.random.default_rng(3)
    h, worst = 1e-6, 0.0
    for _ in range(40):
        Si, Sj = _random_sim3(rng), _random_sim3(rng)
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * 2 * np.tan(np.deg2rad(rng.uniform(0, 10)) / 2)
        err = pg.delta(np.concatenate([w, rng.uniform(-0.5, 0.5, 3), [0.0]]))
        err[7] = np.exp(rng.uniform(-0.2, 0.2))
        M = pg.compose(err, pg.compose(Sj, pg.inverse(Si)))
        ok, r, Ji, Jj = pg.edge_terms(Si, Sj, M, fix_scale)
        assert ok
        for which, J in ((0, Ji), (1, Jj)):
            for k in range(7):
                if fix_scale and k == 6:
                    assert np.all(J[:, 6] == 0.0)
                    continue
                d = np.zeros(7)
                d[k] = h
                rp = pg.residual(pg.retract(Si, d)[1], Sj, M)[1] if which == 0 else pg.residual(Si, pg.retract(Sj, d)[1], M)[1]
                rm = pg.residual(pg.retract(Si, -d)[1], Sj, M)[1] if which == 0 else pg.residual(Si, pg.retract(Sj, -d)[1], M)[1]
                worst = max(worst, np.abs((rp - rm) / (2 * h) - J[:, k]).max())
    print("largest difference from central differences: %.3g" % worst)
    assert worst <= 1e-6


def _scipy_cost(g):
    from scipy.optimize import least_squares
    free = np.flatnonzero(g["fixed"] == 0)
    S0 = np.asarray(g["S"], float)

    def estimate(x):
        S = S0.copy()
        for k, v in enumerate(free):
            ok, S[v] = pg.retract(S0[v], x[7 * k:7 * k + 7])
            assert ok
        return S

    def fun(x):
        S = estimate(x)
        return np.concatenate([pg.residual(S[i], S[j], M)[1] for (i, j), M in zip(g["edges"], g["M"])])
    sol = least_squares(fun, np.zeros(7 * len(free)), method="lm", xtol=1e-14, ftol=1e-14, gtol=1e-14, max_nfev=20000)
    return 2.0 * sol.cost


@pytest.mark.parametrize("n,chords", [(8, 0), (16, 4)])
@pytest.mark.parametrize("noise", [0.0, 0.002])
def test_witness_final_cost_against_scipy(n, chords, noise):
    g = pg.ring(n, chords=chords, noise=noise, seed=11 + n)
    out = pg.optimize(g)
    ref = _scipy_cost(g)
    rel = abs(out["cost_final"] - ref) / ref
    print("ring %d + %d chords, noise %g: cost %.17g -> %.17g, scipy %.17g, relative difference %.3g, %d LM iterations, %d solves, %d CG iterations"
          % (n, chords, noise, out["cost_initial"], out["cost_final"], ref, rel, out["lm_iterations"], out["n_solves"], out["cg_iterations_total"]))
    assert out["status"] != pg.FAILED and out["cost_final"] < out["cost_initial"]
    assert rel <= 1e-6


@pytest.mark.parametrize("kind,n", [("ring", 12), ("star", 12)])
def test_consistent_graph_reaches_the_truth(kind, n):
    g = pg.consistent(n, kind=kind, seed=5)
    out = pg.optimize(g)
    worst = 0.0
    for v in range(n):
        ok, r = pg.lift(pg.compose(out["S"][v], pg.inverse(g["truth"][v])))
        assert ok
        worst = max(worst, np.abs(r).max())
    print("%s %d: cost %.3g -> %.3g, farthest vertex %.3g from the truth, %d LM iterations" % (kind, n, out["cost_initial"], out["cost_final"], worst,
                                                                                          out["lm_iterations"]))
    assert worst <= 1e-8


def test_fix_scale_keeps_every_scale_bit_for_bit():
    g = pg.ring(16, chords=4, noise=0.002, seed=7)
    out = pg.optimize(g, fix_scale=1)
    assert out["status"] != pg.FAILED and out["cost_final"] < out["cost_initial"]
    assert np.array_equal(out["S"][:, 7].view(np.uint64), np.asarray(g["S"])[:, 7].view(np.uint64))
    assert not np.array_equal(out["S"][1:, :7], np.asarray(g["S"])[1:, :7])


def test_zero_residual_component_is_untouched():
    g = pg.with_zero_component(pg.ring(8, seed=3), 3)
    lin = pg.linearize(g)
    assert np.all(lin["res"][-3:] == 0.0)
    out = pg.optimize(g)
    assert out["cost_final"] < out["cost_initial"]
    assert np.array_equal(out["S"][-3:].view(np.uint64), np.asarray(g["S"])[-3:].view(np.uint64))
    assert not np.array_equal(out["S"][1:8], np.asarray(g["S"])[1:8])


@pytest.mark.parametrize("fixed", [(5,), (2, 9)])
def test_fixed_vertices_other_than_the_first(fixed):
    g = pg.ring(12, chords=3, noise=0.002, seed=9, fixed=fixed)
    out = pg.optimize(g)
    ref = _scipy_cost(g)
    assert abs(out["cost_final"] - ref) / ref <= 1e-6
    S0 = np.asarray(g["S"])
    for v in range(12):
        same = np.array_equal(out["S"][v].view(np.uint64), S0[v].view(np.uint64))
        assert same == (v in fixed), v


def test_cg_cap_never_raises_the_cost_and_is_counted():
    g = pg.ring(16, seed=4)
    out = pg.optimize(g, cg_max_iterations=5)
    assert out["cg_capped"] >= 1 and out["cg_iterations_total"] <= 5 * out["n_solves"]
    assert out["cost_final"] <= out["cost_initial"]
    costs = [pg.optimize(g, cg_max_iterations=5, max_iterations=k)["cost_final"] for k in range(1, 8)]
    assert all(b <= a for a, b in zip([out["cost_initial"]] + costs, costs)), costs


def test_failure_at_the_initial_estimate_returns_the_input():
    """an edge whose error is a rotation of exactly 180 degrees (w = 0): status failed, nothing moved"""
    S = np.array([[1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, 1, 1, 0, 0, 1]], np.float64)
    g = dict(S=S, fixed=np.array([0, 1, 0], np.uint8), edges=np.array([(0, 1), (1, 2)], np.int32), M=np.array([pg.IDENTITY, pg.IDENTITY]))
    assert not pg.linearize(g)["ok"]
    out = pg.optimize(g)
    assert out["status"] == pg.FAILED and out["lm_iterations"] == 0 and np.array_equal(out["S"], S)
