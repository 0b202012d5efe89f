"""The restatement of the relocalisation pose solver (tests/pnp_ref.c) against ground truth, without a device: Lambda Twist P3P recovers
the true pose of noise-free general and planar triples, never returns more than 4 solutions, returns none (and no NaN) for degenerate
triples; RANSAC on 600 noise-free points with 30 % and 60 % outliers finds the exact inlier set and the pose; the sample sets follow
cv::RNG's scheme of Initializer.cpp:33-49 with 3 indices."""
import numpy as np
import pytest

import pnp_ref as pr


def _pose_err(S, R, t):
    return max(np.abs(S[:9].reshape(3, 3) - R).max(), np.abs(S[9:] - t).max())


def _well_conditioned(pw3, px3):
    """triangles whose smallest angle (world) is above 15 degrees and whose pixels lie 40 px apart: the 1e-9 tolerance is for those"""
    ang = []
    for i in range(3):
        a, b = pw3[(i + 1) % 3] - pw3[i], pw3[(i + 2) % 3] - pw3[i]
        ang.append(np.degrees(np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1))))
    d = min(np.linalg.norm(px3[i] - px3[j]) for i in range(3) for j in range(i + 1, 3))
    return min(ang) > 15 and d > 40


@pytest.mark.parametrize("planar", [False, True])
def test_p3p_recovers_the_true_pose_of_noise_free_triples(planar):
    tried = 0
    for seed in range(600):
        sc = pr.scene(3, seed, planar=planar)
        if not _well_conditioned(sc["pw"], sc["px"]):
            continue
        tried += 1
        n, sol = pr.p3p(sc["pw"], sc["px"], sc["K4"])
        assert 1 <= n <= 4, (seed, n)
        assert np.isfinite(sol).all()
        err = min(_pose_err(S, sc["R"], sc["t"]) for S in sol)
        assert err < 1e-9, (seed, err)
        for S in sol:                                      # every solution is a rotation
            R = S[:9].reshape(3, 3)
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-8 and np.linalg.det(R) > 0
    assert tried > 100


def test_solution_count_never_exceeds_four():
    rng = np.random.default_rng(3)
    counts = []
    for _ in range(3000):                                  # random triples, random pixels: most have no consistent pose at all
        n, _ = pr.p3p(rng.uniform(-2, 2, (3, 3)) + [0, 0, 4], rng.uniform(0, 640, (3, 2)), pr.K4_DEFAULT)
        counts.append(n)
    assert max(counts) <= 4 and min(counts) >= 0 and max(counts) >= 2


def test_degenerate_triples_give_no_solution_and_no_nan():
    K4 = pr.K4_DEFAULT
    px = np.array([[100.0, 100.0], [300.0, 200.0], [500.0, 50.0]])
    for pw in [np.array([[0, 0, 4.0], [1, 1, 5.0], [2, 2, 6.0]]),       # collinear
               np.array([[0, 0, 4.0], [0, 0, 4.0], [1, 0, 4.0]]),       # two coincident
               np.array([[1, 2, 3.0]] * 3)]:                            # all coincident
        n, sol = pr.p3p(pw, px, K4)
        assert n == 0 and not np.isnan(sol).any()
    # the same pixel three times, a general triangle: no NaN in whatever comes back, and RANSAC over such points scores 0 without a NaN
    n, sol = pr.p3p(np.array([[0, 0, 4.0], [1, 0, 4.0], [0, 1, 4.0]]), np.array([[320.0, 240.0]] * 3), K4)
    assert np.isfinite(sol).all()
    pw = np.tile([[1.0, 2.0, 3.0]], (20, 1))
    r = pr.ransac(pw, np.tile([[320.0, 240.0]], (20, 1)), K4, max_iter=50)
    assert r["result"]["success"] == 0 and r["result"]["best_sample"] == -1 and r["result"]["n_hypotheses"] == 0
    assert np.isfinite(r["solutions"]).all() and r["counts"].max() == 0 and not r["inliers"].any()
    assert np.array_equal(r["result"]["T_cw"], [0, 0, 0, 1, 0, 0, 0])


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("outliers", [0.3, 0.6])
def test_ransac_recovers_the_exact_inlier_set_and_pose(planar, outliers):
    sc = pr.scene(600, 40 + int(outliers * 10) + planar, planar=planar, outliers=outliers)
    r = pr.ransac(sc["pw"], sc["px"], sc["K4"])
    # the exact inlier set: the points within the threshold under the true pose (an outlier pixel may land within 2.4 px of its projection)
    truth = np.sum((pr.project(sc["K4"], sc["pw"] @ sc["R"].T + sc["t"]) - sc["px"]) ** 2, 1) <= 5.991
    assert np.array_equal(r["inliers"], truth)
    assert r["result"]["success"] == 1 and r["result"]["n_inliers"] == truth.sum()
    assert np.abs(r["result"]["R"].reshape(3, 3) - sc["R"]).max() < 1e-9 and np.abs(r["result"]["t"] - sc["t"]).max() < 1e-9
    q = r["result"]["T_cw"][:4]                            # the quaternion of R
    x, y, z, w = q
    Rq = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    assert np.abs(Rq - sc["R"]).max() < 1e-9 and np.array_equal(r["result"]["T_cw"][4:], r["result"]["t"])
    # the winner is the first hypothesis of the highest count
    c = r["counts"].reshape(-1)
    assert c.max() == r["result"]["n_inliers"] and int(np.argmax(c)) == 4 * r["result"]["best_sample"] + r["result"]["best_solution"]
    assert r["result"]["n_hypotheses"] == r["n_solutions"].sum()


def _cv_rng_sets(n, max_iter, k=3):
    """cv::RNG (state 0xffffffff, multiply-with-carry, uniform(0, m) = next() % m) and the swap-remove of availableIndices, in Python"""
    st, out = 0xffffffff, []
    for _ in range(max_iter):
        avail = list(range(n))
        row = []
        for _ in range(k):
            st = ((st & 0xffffffff) * 4164903690 + (st >> 32)) & 0xffffffffffffffff
            r = (st & 0xffffffff) % len(avail)
            row.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        out.append(row)
    return np.array(out, np.int32)


@pytest.mark.parametrize("n", [4, 5, 50, 600, 3072])
def test_sample_sets_follow_the_scheme(n):
    s = pr.sample_sets(n, 300)
    assert s.shape == (300, 3)
    assert np.array_equal(s, pr.sample_sets(n, 300))
    assert all(len(set(row)) == 3 for row in s.tolist()) and s.min() >= 0 and s.max() < n
    assert np.array_equal(s, _cv_rng_sets(n, 300))


def test_cubic_root_is_the_largest_real_root():
    rng = np.random.default_rng(1)
    for _ in range(500):
        b, c, d = rng.normal(0, 10, 3)
        x = pr.cubic_root(b, c, d)
        roots = np.roots([1, b, c, d])
        real = roots[np.abs(roots.imag) < 1e-7].real
        assert abs(x - real.max()) <= 1e-7 * max(1, abs(x)), (b, c, d, x, real)
