"""The Sim3 pose-graph optimiser on the MI355X (ygz_hip_pose_graph_optimize / ygz_hip_pgo_linearize, ygz_slam_amd/csrc/pgo.hip) against its
restatement tests/pgo_ref.c, bit for bit: S_out, both costs, lambda, the iteration, solve and CG counters and the status, on the smallest
shapes where the kernel can go wrong -- one edge, rings with chords and noise, a star (one vertex of degree 39), more unknowns than lanes
(7 N > 256), more edges and unknowns than 1024 with the CG cap exercised, fix_scale, two fixed vertices, a zero-residual component; the stage
export's residuals and Jacobians; one refusal through a live context."""
import numpy as np
import pytest

import pgo_ref as pg

pytestmark = pytest.mark.gpu

FIELDS = ["status", "lm_iterations", "n_solves", "cg_iterations_total", "cg_capped", "cost_initial", "cost_final", "lambda_"]


def _star(n):
    g = pg.consistent(n, kind="star", seed=40)
    rng = np.random.default_rng(41)
    g["M"] = np.array([pg.compose(pg.delta(rng.normal(0, 0.01, 7)), M) for M in g["M"]])      # inconsistent: the optimum is not the truth
    return g


def _two(seed=2):
    g = pg.consistent(2, kind="star", seed=seed)
    return g


SHAPES = {
    "n2_e1": (lambda: _two(), {}),
    "ring8": (lambda: pg.ring(8, seed=19), {}),
    "ring16_chords4_noise": (lambda: pg.ring(16, chords=4, noise=0.002, seed=27), {}),
    "star40": (lambda: _star(40), {}),
    "ring64_chords16": (lambda: pg.ring(64, chords=16, noise=0.001, seed=64), {}),
    "ring300_chords100_cap200": (lambda: pg.ring(300, chords=100, noise=0.001, seed=300), dict(cg_max_iterations=200, max_iterations=4)),
    "fix_scale": (lambda: pg.ring(16, chords=4, noise=0.002, seed=7), dict(fix_scale=1)),
    "two_fixed": (lambda: pg.ring(12, chords=3, noise=0.002, seed=9, fixed=(2, 9)), {}),
    "zero_component": (lambda: pg.with_zero_component(pg.ring(8, seed=3), 3), {}),
}


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """every shape's graph and the restatement's answer, computed once"""
    out = {}
    for name, (make, kw) in SHAPES.items():
        g = make()
        out[name] = (g, kw, pg.optimize(g, **kw), pg.linearize(g, fix_scale=bool(kw.get("fix_scale", 0))))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_the_restatement(ctx, cases, name):
    g, kw, ref, _ = cases[name]
    dev = ctx.pose_graph_optimize(g["S"], g["fixed"], g["edges"], g["M"], **kw)
    print("%s: N %d E %d, cost %.6g -> %.6g, status %d, %d LM iterations, %d solves, %d CG iterations, %d capped"
          % (name, len(g["S"]), len(g["edges"]), ref["cost_initial"], ref["cost_final"], ref["status"], ref["lm_iterations"], ref["n_solves"],
             ref["cg_iterations_total"], ref["cg_capped"]))
    for k in FIELDS:
        assert _bits([dev[k]])[0] == _bits([ref[k]])[0] if isinstance(ref[k], float) else dev[k] == ref[k], (k, dev[k], ref[k])
    assert np.array_equal(_bits(dev["S"]), _bits(ref["S"]))
    assert ref["status"] != pg.FAILED and ref["cost_final"] < ref["cost_initial"]
    if name == "ring300_chords100_cap200":
        assert ref["cg_capped"] >= 1
    if name == "fix_scale":
        assert np.array_equal(_bits(dev["S"][:, 7]), _bits(np.asarray(g["S"])[:, 7]))
    if name == "zero_component":
        assert np.array_equal(_bits(dev["S"][-3:]), _bits(np.asarray(g["S"])[-3:]))
    if name == "two_fixed":
        assert np.array_equal(_bits(dev["S"][[2, 9]]), _bits(np.asarray(g["S"])[[2, 9]]))


@pytest.mark.parametrize("name", ["n2_e1", "ring16_chords4_noise", "ring300_chords100_cap200", "fix_scale"])
def test_stage_export_equals_the_restatement(ctx, cases, name):
    g, kw, _, ref = cases[name]
    dev = ctx.pgo_linearize(g["S"], g["fixed"], g["edges"], g["M"], **kw)
    assert dev["ok"] and ref["ok"]
    for k in ["res", "Ji", "Jj"]:
        assert np.array_equal(_bits(dev[k]), _bits(ref[k])), k
    assert _bits([dev["cost"]])[0] == _bits([ref["cost"]])[0]


def test_failure_at_the_initial_estimate(ctx):
    S = np.array([[1, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, 1, 1, 0, 0, 1]], np.float64)
    g = dict(S=S, fixed=np.array([0, 1, 0], np.uint8), edges=np.array([(0, 1), (1, 2)], np.int32), M=np.array([pg.IDENTITY, pg.IDENTITY]))
    dev, ref = ctx.pose_graph_optimize(g["S"], g["fixed"], g["edges"], g["M"]), pg.optimize(g)
    assert dev["status"] == ref["status"] == pg.FAILED and dev["lm_iterations"] == 0
    assert np.array_equal(_bits(dev["S"]), _bits(S))
    assert not ctx.pgo_linearize(g["S"], g["fixed"], g["edges"], g["M"])["ok"]


def test_refusal_through_a_live_context(ctx, hip_lib, cases):
    g = cases["ring8"][0]
    edges = np.array(g["edges"]).copy()
    edges[3] = (4, 4)
    with pytest.raises(hip_lib.YgzHipError) as e:
        ctx.pose_graph_optimize(g["S"], g["fixed"], edges, g["M"])
    assert e.value.code == hip_lib.E_INVALID
    out = ctx.pose_graph_optimize(g["S"], g["fixed"], g["edges"], g["M"])                     # the context is still good
    assert out["status"] != hip_lib.PGO_FAILED
