"""The relocalisation's P3P RANSAC on the MI355X (ygz_hip_pnp_ransac / ygz_hip_pnp_hypotheses, ygz_slam_amd/csrc/pnp.hip) against its
restatement tests/pnp_ref.c: every hypothesis's solutions, the solution counts and the per-hypothesis inlier counts, the winner, its mask and
T_cw bit for bit on general and planar scenes of 4 to 3072 points with 0, 30 and 60 % outliers; a 5-problem call equal to 5 single calls;
degenerate and all-outlier problems fail without a fault; K4 and chi2 honoured; capacities refused."""
import numpy as np
import pytest

import pnp_ref as pr

pytestmark = pytest.mark.gpu

SCENES = [(n, planar, out) for n in (4, 50, 600, 3072) for planar in (False, True) for out in (0.0, 0.3, 0.6)]
FIELDS = ["success", "n_inliers", "best_sample", "best_solution", "n_hypotheses"]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


def _scene(n, planar, out, seed=0):
    return pr.scene(n, 1000 + 7 * n + 3 * planar + int(out * 10) + seed, planar=planar, noise=0.3, outliers=out)


def _same(a, b):
    for k in FIELDS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ["R", "t", "T_cw"]:
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])


@pytest.mark.parametrize("n,planar,out", SCENES)
def test_device_equals_the_restatement(ctx, n, planar, out):
    sc = _scene(n, planar, out)
    ref = pr.ransac(sc["pw"], sc["px"], sc["K4"])
    hyp = ctx.pnp_hypotheses(sc["pw"], sc["px"], sc["K4"])
    assert np.array_equal(hyp["n_solutions"], ref["n_solutions"])
    assert np.array_equal(hyp["solutions"], ref["solutions"])
    assert np.array_equal(hyp["counts"], ref["counts"])
    res, inl = ctx.pnp_ransac(sc["pw"], sc["px"], [0, n], sc["K4"])
    _same(res[0], ref["result"])
    assert np.array_equal(inl, ref["inliers"])
    if n >= 50 and out <= 0.3:                             # enough all-inlier samples: the pose is found
        assert res[0]["success"] == 1
        assert np.abs(res[0]["R"].reshape(3, 3) - sc["R"]).max() < 5e-2 and np.abs(res[0]["t"] - sc["t"]).max() < 0.1


def test_five_problems_equal_five_calls(ctx):
    scs = [_scene(n, planar, out, seed=5) for n, planar, out in [(50, False, 0.3), (600, True, 0.6), (4, False, 0.0), (3072, True, 0.3),
                                                                 (200, False, 0.0)]]
    pw = np.concatenate([s["pw"] for s in scs]); px = np.concatenate([s["px"] for s in scs])
    off = np.concatenate([[0], np.cumsum([len(s["pw"]) for s in scs])])
    res, inl = ctx.pnp_ransac(pw, px, off, pr.K4_DEFAULT)
    for p, s in enumerate(scs):
        r1, i1 = ctx.pnp_ransac(s["pw"], s["px"], [0, len(s["pw"])], pr.K4_DEFAULT)
        _same(res[p], r1[0])
        assert np.array_equal(inl[off[p]:off[p + 1]], i1)


def test_degenerate_and_all_outlier_problems_fail_cleanly(ctx):
    rng = np.random.default_rng(2)
    n = 100
    collinear = np.stack([np.linspace(-1, 1, n), np.linspace(-1, 1, n) * 0.5, np.full(n, 3.0)], 1)
    same = np.tile([[0.1, 0.2, 3.0]], (n, 1))
    px = rng.uniform(0, 640, (n, 2))
    sc = _scene(300, False, 0.0)
    junk = rng.uniform(0, 640, (300, 2))                   # every correspondence an outlier
    pw = np.concatenate([collinear, same, sc["pw"]]); pxs = np.concatenate([px, px, junk])
    res, inl = ctx.pnp_ransac(pw, pxs, [0, n, 2 * n, 2 * n + 300], pr.K4_DEFAULT)
    for p, (w, x) in enumerate([(collinear, px), (same, px), (sc["pw"], junk)]):
        ref = pr.ransac(w, x, pr.K4_DEFAULT)
        _same(res[p], ref["result"])
        assert res[p]["success"] == 0 and np.isfinite(res[p]["T_cw"]).all()
    assert res[0]["n_hypotheses"] == 0 and res[1]["n_hypotheses"] == 0 and res[0]["best_sample"] == -1
    assert not inl[:2 * n].any()


def test_k4_and_chi2_are_honoured(ctx):
    K4 = np.array([400.0, 410.0, 300.0, 260.0])
    sc = pr.scene(600, 77, planar=True, noise=0.8, outliers=0.3, K4=K4)
    for chi2, it in [(1.0, 300), (5.991, 64), (20.0, 1024)]:
        ref = pr.ransac(sc["pw"], sc["px"], K4, chi2=chi2, max_iter=it, min_inliers=400)
        res, inl = ctx.pnp_ransac(sc["pw"], sc["px"], [0, 600], K4, chi2=chi2, max_iter=it, min_inliers=400)
        _same(res[0], ref["result"])
        assert np.array_equal(inl, ref["inliers"])
    a, _ = ctx.pnp_ransac(sc["pw"], sc["px"], [0, 600], K4, chi2=1.0)
    b, _ = ctx.pnp_ransac(sc["pw"], sc["px"], [0, 600], K4, chi2=20.0)
    c, _ = ctx.pnp_ransac(sc["pw"], sc["px"], [0, 600], pr.K4_DEFAULT, chi2=20.0)
    assert a[0]["n_inliers"] < b[0]["n_inliers"] and c[0]["n_inliers"] < b[0]["n_inliers"]


def test_capacities_and_bad_arguments_are_refused(ctx, hip_lib):
    sc = _scene(50, False, 0.0)
    pw = np.tile(sc["pw"], (65, 1)); px = np.tile(sc["px"], (65, 1))
    with pytest.raises(hip_lib.YgzHipError) as e:
        ctx.pnp_ransac(pw, px, np.arange(66) * 50, pr.K4_DEFAULT)
    assert e.value.code == hip_lib.E_CAPACITY
    big = pr.scene(ctx.cells + 1, 1)
    with pytest.raises(hip_lib.YgzHipError) as e:
        ctx.pnp_ransac(big["pw"], big["px"], [0, ctx.cells + 1], pr.K4_DEFAULT)
    assert e.value.code == hip_lib.E_CAPACITY
    for kw, off in [(dict(max_iter=0), [0, 50]), (dict(max_iter=1025), [0, 50]), (dict(chi2=0.0), [0, 50]), ({}, [0, 3]), ({}, [1, 50])]:
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.pnp_ransac(sc["pw"], sc["px"], off, pr.K4_DEFAULT, **kw)
        assert e.value.code == hip_lib.E_INVALID
