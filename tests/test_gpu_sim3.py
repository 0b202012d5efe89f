"""The loop detection's Sim3 RANSAC and refinement on the MI355X (ygz_hip_sim3_ransac / ygz_hip_sim3_hypotheses, ygz_slam_amd/csrc/sim3.hip)
against its restatement tests/sim3_ref.c: every sample's S12 / S21, validity and count, the winner, its mask, the refined S12 / S21, refined
mask and chi2 bit for bit on scenes of 3 to 3072 pairs, 1, 5 and 64 problems per call, with and without fix_scale; an all-degenerate problem
gives no winner and no NaN; bad arguments and capacities are refused."""
import numpy as np
import pytest

import sim3_ref as sr

pytestmark = pytest.mark.gpu

SIZES = [3, 20, 200, 1000, 3072]
INT_FIELDS = ["success", "n_hypotheses", "best_sample", "n_inliers", "n_refined", "lm_iterations"]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


def _same(a, b):
    for k in INT_FIELDS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ["S12", "S21", "chi2_ransac", "chi2_refined"]:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (k, a[k], b[k])


def _call(ctx, scs, **kw):
    cat = lambda k: np.concatenate([s[k] for s in scs])
    off = np.concatenate([[0], np.cumsum([len(s["X1"]) for s in scs])])
    res, mask = ctx.sim3_ransac(cat("X1"), cat("X2"), cat("px1"), cat("px2"), cat("levels"), off, scs[0]["K4"], **kw)
    return res, mask, off


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_device_equals_the_restatement(ctx, n, fix):
    sc = sr.scene(n, 500 + n + fix, outliers=0.3, fix_scale=bool(fix))
    ref = sr.ransac(sc, fix_scale=fix)
    hyp = ctx.sim3_hypotheses(sc["X1"], sc["X2"], sc["px1"], sc["px2"], sc["levels"], sc["K4"], fix_scale=fix)
    assert np.array_equal(hyp["valid"], ref["valid"])
    assert np.array_equal(hyp["hyps"], ref["hyps"])
    assert np.array_equal(hyp["counts"], ref["counts"])
    res, mask, _ = _call(ctx, [sc], fix_scale=fix)
    _same(res[0], ref["result"])
    assert np.array_equal(mask, ref["mask"])
    if n >= 200:
        r = res[0]
        assert r["success"] == 1 and r["n_refined"] >= 20 and np.isfinite(r["S12"]).all()
        assert abs(r["S12"][7] - sc["S12"][7]) < 0.02 * sc["S12"][7] and np.abs(r["S12"][4:7] - sc["S12"][4:7]).max() < 0.05
        if fix:
            assert r["S12"][7] == 1.0


@pytest.mark.parametrize("P", [5, 64])
def test_many_problems_equal_the_restatement(ctx, P):
    rng = np.random.default_rng(P)
    sizes = [int(v) for v in rng.choice([3, 20, 200, 1000], P)]
    if P == 5:
        sizes = [200, 3, 1000, 20, 3072]
    scs = [sr.scene(n, 900 + 13 * k + n, outliers=float(rng.choice([0.0, 0.3, 0.6]))) for k, n in enumerate(sizes)]
    res, mask, off = _call(ctx, scs)
    for p, s in enumerate(scs):
        ref = sr.ransac(s)
        _same(res[p], ref["result"])
        assert np.array_equal(mask[off[p]:off[p + 1]], ref["mask"]), p


def test_degenerate_problem_gives_no_winner_and_no_nan(ctx):
    n = 60
    line = np.stack([np.linspace(-1, 1, n), np.linspace(-1, 1, n) * 0.3, np.full(n, 3.0)], 1)
    same = np.tile([[0.1, 0.2, 3.0]], (n, 1))
    px = np.random.default_rng(3).uniform(0, 640, (n, 2))
    lv = np.zeros((n, 2), np.int32)
    good = sr.scene(300, 71)
    scs = [dict(X1=line, X2=line * 1.1, px1=px, px2=px, levels=lv, K4=sr.K4_DEFAULT),
           dict(X1=same, X2=same, px1=px, px2=px, levels=lv, K4=sr.K4_DEFAULT), good]
    res, mask, off = _call(ctx, scs)
    for p in (0, 1):
        ref = sr.ransac(scs[p])
        _same(res[p], ref["result"])
        r = res[p]
        assert r["n_hypotheses"] == 0 and r["best_sample"] == -1 and r["success"] == 0 and r["n_refined"] == 0
        assert np.array_equal(r["S12"], [0, 0, 0, 1, 0, 0, 0, 1]) and np.isfinite(r["S21"]).all()
    assert not mask[:off[2]].any()
    _same(res[2], sr.ransac(good)["result"])


def test_bad_arguments_and_capacities_are_refused(ctx, hip_lib):
    sc = sr.scene(50, 5)
    args = [sc[k] for k in ("X1", "X2", "px1", "px2", "levels")]
    tile = [np.tile(a, (65, 1)) for a in args]
    with pytest.raises(hip_lib.YgzHipError) as e:
        ctx.sim3_ransac(*tile, np.arange(66) * 50, sr.K4_DEFAULT)
    assert e.value.code == hip_lib.E_CAPACITY
    big = sr.scene(ctx.cells + 1, 6)
    with pytest.raises(hip_lib.YgzHipError) as e:
        ctx.sim3_ransac(*[big[k] for k in ("X1", "X2", "px1", "px2", "levels")], [0, ctx.cells + 1], sr.K4_DEFAULT)
    assert e.value.code == hip_lib.E_CAPACITY
    for kw, off in [(dict(max_iter=0), [0, 50]), (dict(max_iter=1025), [0, 50]), (dict(chi2=0.0), [0, 50]), (dict(chi2_refine=-1.0), [0, 50]),
                    ({}, [0, 2, 50]), ({}, [1, 50])]:
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.sim3_ransac(*args, off, sr.K4_DEFAULT, **kw)
        assert e.value.code == hip_lib.E_INVALID, (kw, off)
