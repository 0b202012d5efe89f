"""tests/sim3_ref.c, the restatement of the loop detection's Sim3 solver, against ground truth and independent witnesses: Horn's closed form
on exact samples, against a numpy Umeyama (SVD) fit, degenerate samples, fix_scale, RANSAC under outliers, the refinement's analytic
Jacobians against central differences, Sigma rho never raised by the LM, and the sample sets of the P3P RANSAC."""
import numpy as np
import pytest

import sim3_ref as sr


def _umeyama(X1, X2, fix_scale=False):
    """S12 = (R, t, s) minimising sum |X1 - s R X2 - t|^2 (Umeyama 1991), the scale of Horn's asymmetric form for comparison"""
    m1, m2 = X1.mean(0), X2.mean(0)
    A, B = X1 - m1, X2 - m2
    U, _, Vt = np.linalg.svd(A.T @ B)
    D = np.eye(3)
    D[2, 2] = np.sign(np.linalg.det(U @ Vt))
    R = U @ D @ Vt
    RB = B @ R.T
    s = 1.0 if fix_scale else float((A * RB).sum() / (RB * RB).sum())
    return R, m1 - s * R @ m2, s


def test_exact_samples_recover_the_sim3():
    rng = np.random.default_rng(1)
    for _ in range(200):
        S = sr.random_sim3(rng, scale=(0.2, 5.0), deg=(0, 170), t=2.0)
        X2 = rng.normal(size=(3, 3)) * rng.uniform(0.1, 3) + rng.normal(size=3) * 3
        X1 = sr.act(S, X2)
        ok, S12, S21 = sr.solve3(X1, X2)
        assert ok
        q = S12[:4] if np.dot(S12[:4], S[:4]) >= 0 else -S12[:4]
        assert np.abs(q - S[:4]).max() < 1e-12 * 100 and S12[3] >= 0
        assert abs(S12[7] - S[7]) < 1e-12 * S[7] * 100
        assert np.abs(sr.act(S12, X2) - X1).max() < 1e-12 * max(1.0, np.abs(X1).max()) * 100
        assert np.abs(sr.act(S21, X1) - X2).max() < 1e-12 * max(1.0, np.abs(X2).max()) * 100
        # the direction: R12 Pr2 ~ Pr1
        R = sr.quat_to_R(S12[:4])
        assert np.abs((X2 - X2.mean(0)) @ R.T * S12[7] - (X1 - X1.mean(0))).max() < 1e-10


def test_n_points_agree_with_umeyama():
    rng = np.random.default_rng(2)
    for fix in (False, True):
        for n in (3, 10, 100, 1000):
            S = sr.random_sim3(rng, scale=(1.0, 1.0) if fix else (0.5, 2.0))
            X2 = rng.normal(size=(n, 3)) + [0, 0, 4]
            X1 = sr.act(S, X2) + rng.normal(0, 0.01, (n, 3))
            ok, S12, _ = sr.horn(X1, X2, fix_scale=fix)
            R, t, s = _umeyama(X1, X2, fix)
            assert ok
            assert np.abs(sr.quat_to_R(S12[:4]) - R).max() < 1e-9 and np.abs(S12[4:7] - t).max() < 1e-9 and abs(S12[7] - s) < 1e-9


def test_degenerate_samples_are_invalid_without_nan():
    line = np.array([[0, 0, 1.0], [1, 1, 2.0], [2, 2, 3.0]])
    tri = np.array([[0, 0, 3.0], [1, 0, 3.0], [0, 1, 4.0]])
    same = np.tile([[0.5, 0.5, 2.0]], (3, 1))
    two = np.array([[0, 0, 1.0], [0, 0, 1.0], [1, 0, 1.0]])
    for a, b in [(line, tri), (tri, line), (same, tri), (tri, same), (two, tri), (tri, np.zeros((3, 3)))]:
        ok, S12, S21 = sr.solve3(a, b)
        assert ok == 0
        assert np.array_equal(S12, [0, 0, 0, 1, 0, 0, 0, 1]) and np.array_equal(S21, S12)
    # a mirrored triple (negative scale is impossible: s = sum Pr1.R Pr2 / sum |R Pr2|^2 > 0 for a proper rotation), and NaN input
    nan = tri.copy(); nan[1, 2] = np.nan
    ok, S12, _ = sr.solve3(nan, tri)
    assert ok == 0 and np.isfinite(S12).all()


def test_fix_scale_gives_unit_scale_exactly():
    rng = np.random.default_rng(3)
    for _ in range(50):
        S = sr.random_sim3(rng)
        X2 = rng.normal(size=(3, 3)) + [0, 0, 3]
        ok, S12, S21 = sr.solve3(sr.act(S, X2), X2, fix_scale=True)
        assert ok and S12[7] == 1.0 and S21[7] == 1.0
    sc = sr.scene(500, 4, fix_scale=True)
    r = sr.ransac(sc, fix_scale=1)["result"]
    assert r["success"] == 1 and r["S12"][7] == 1.0 and r["S21"][7] == 1.0


@pytest.mark.parametrize("n,seed", [(200, 10), (1000, 11), (3072, 12)])
def test_ransac_recovers_the_sim3_under_outliers(n, seed):
    sc = sr.scene(n, seed, noise=0.5, outliers=0.3)
    o = sr.ransac(sc)
    r, mask = o["result"], o["mask"]
    assert r["success"] == 1 and r["best_sample"] >= 0 and r["n_hypotheses"] > 250
    S, T = r["S12"], sc["S12"]
    assert abs(S[7] / T[7] - 1) < 0.01 and np.abs(S[4:7] - T[4:7]).max() < 0.01
    assert np.degrees(2 * np.arccos(min(1.0, abs(np.dot(S[:4], T[:4]))))) < 0.25
    ransac_in, refined = (mask & 1).astype(bool), (mask & 2).astype(bool)
    assert ransac_in.sum() == r["n_inliers"] and refined.sum() == r["n_refined"]
    assert not (refined & ~ransac_in).any()
    assert (refined & sc["outlier"]).sum() <= 0.02 * n and refined.sum() >= 0.9 * (~sc["outlier"]).sum()
    assert np.array_equal(o["counts"], np.where(o["valid"] != 0, o["counts"], 0))


def test_jacobians_agree_with_central_differences():
    rng = np.random.default_rng(5)
    K4 = sr.K4_DEFAULT
    for fix in (0, 1):
        for _ in range(20):
            S = sr.random_sim3(rng, scale=(1.0, 1.0) if fix else (0.5, 2.0))
            X1 = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(2, 5)])
            X2 = ((X1 - S[4:7]) @ sr.quat_to_R(S[:4])) / S[7] + rng.normal(0, 0.05, 3)
            u1, u2 = rng.uniform(100, 500, 2), rng.uniform(100, 400, 2)
            t = sr.pair_terms(S, X1, X2, u1, u2, 1, 2, K4, fix)
            for k in range(7 - fix):
                h = 1e-6
                d = np.zeros(7); d[k] = h
                okp, Sp = sr.apply_delta(S, d)
                okm, Sm = sr.apply_delta(S, -d)
                assert okp and okm
                tp = sr.pair_terms(Sp, X1, X2, u1, u2, 1, 2, K4, fix)
                tm = sr.pair_terms(Sm, X1, X2, u1, u2, 1, 2, K4, fix)
                for e, J in (("e12", "J12"), ("e21", "J21")):
                    num = (tp[e] - tm[e]) / (2 * h)
                    ana = t[J][:, k]
                    assert np.abs(num - ana).max() <= 1e-6 * max(1.0, np.abs(ana).max()), (fix, k, e, num, ana)
            if fix:
                assert np.array_equal(t["J12"][:, 6], [0, 0]) and np.array_equal(t["J21"][:, 6], [0, 0])
    assert sr.apply_delta(sr.random_sim3(rng), [0, 0, 0, 0, 0, 0, 2.0])[0] == 0


def _sum_rho(sc, S, sel, fix, th2=10.0):
    """g2o's Huber cost of both edges of the pairs sel at S (numpy side of sr_accumulate)"""
    tot = 0.0
    for i in np.flatnonzero(sel):
        t = sr.pair_terms(S, sc["X1"][i], sc["X2"][i], sc["px1"][i], sc["px2"][i], sc["levels"][i, 0], sc["levels"][i, 1], sc["K4"], fix)
        for c in (t["c12"], t["c21"]):
            tot += c if c <= th2 else 2 * np.sqrt(th2) * np.sqrt(c) - th2
    return tot


def test_lm_never_raises_the_cost():
    for seed in range(6):
        for fix in (0, 1):
            sc = sr.scene(300, 300 + seed, noise=1.0, outliers=0.3, fix_scale=bool(fix))
            r = sr.ransac(sc, fix_scale=fix)["result"]
            assert r["n_inliers"] >= 20
            assert r["chi2_refined"] <= r["chi2_ransac"] and r["lm_iterations"] >= 2
            # the first round after k = 0, 1, ... iterations (a second round of 0 iterations leaves S12 where the first ended)
            costs = []
            for k in range(0, 7):
                o = sr.ransac(sc, fix_scale=fix, iters_first=k, iters_more=0, iters_again=0)
                costs.append(_sum_rho(sc, o["result"]["S12"], (o["mask"] & 1).astype(bool), fix))
            assert np.isclose(costs[0], r["chi2_ransac"], rtol=1e-12)
            assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:])), costs
            assert costs[-1] < costs[0]


def test_sample_sets_equal_pnp_sample_sets(hip_lib):
    for n in (4, 20, 600, 3072):
        assert np.array_equal(sr.sample_sets(n, 300), hip_lib.pnp_sample_sets(n, 300))
    s = sr.sample_sets(3, 10)
    assert all(sorted(r) == [0, 1, 2] for r in s.tolist())
