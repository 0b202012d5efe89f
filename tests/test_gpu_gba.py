"""The global bundle adjustment on the MI355X (ygz_hip_global_ba / ygz_hip_gba_linearize, ygz_slam_amd/csrc/gba.hip) against its restatement
tests/gba_ref.c, bit for bit: the poses, the points, both costs, lambda, the status and every counter, on the smallest shapes where the
kernels can go wrong -- the minimum problem, points of exactly 2 and 3 observations, more points than a workgroup's lanes with 300 edges per
pose (partial wavefronts, a partial tree), more free poses than the resident LM takes, 6 N > 256 with the CG cap hit and with batches of 1
and of 64 CG iterations per read-back, the Huber kernel on (10 % outliers) and off, two fixed poses, a repeated edge, exact data at the
truth, a point behind a camera, trials that are rejected; the stage export's residuals, weights, Jacobian blocks, system blocks and cost; one
refusal through a live context."""
import numpy as np
import pytest

import gba_ref as gb
from test_gba_ref import _lattice

pytestmark = pytest.mark.gpu

FIELDS = ["status", "lm_iterations", "n_solves", "cg_iterations_total", "cg_capped", "cost_initial", "cost_final", "lambda_"]

# name -> (the problem, the parameters)
SHAPES = {
    "p2_l8": (lambda: gb.scene(2, 8, 2, seed=31), {}),
    "p3_obs2_obs3": (lambda: gb.scene(3, 12, (2, 3), seed=32), {}),
    "p4_l300": (lambda: gb.scene(4, 300, 4, seed=33), {}),
    "p24_l400": (lambda: gb.scene(24, 400, 4, seed=34), {}),
    "p48_l600_cap": (lambda: gb.scene(48, 600, 4, seed=35), dict(cg_max_iterations=12, max_iterations=4)),
    "huber_outliers": (lambda: gb.scene(8, 80, 4, outliers=0.1, seed=24, fixed=(0, 4)), {}),
    "huber_off": (lambda: gb.scene(8, 80, 4, outliers=0.1, seed=24, fixed=(0, 4), huber=0.0), {}),
    "two_fixed": (lambda: gb.scene(6, 60, 3, seed=27, fixed=(1, 4)), {}),
    "repeated_edge": (lambda: gb.scene(4, 30, 3, seed=25, repeat_edge=True), {}),
    "exact_at_truth": (_lattice, {}),
    "rejected_trials": (lambda: gb.scene(4, 30, 3, seed=25), dict(max_iterations=30, min_rel_decrease=0.0)),
}


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """every shape's problem and the restatement's answers, computed once"""
    out = {}
    for name, (make, kw) in SHAPES.items():
        g = make()
        out[name] = (g, kw, gb.optimize(g, **kw), gb.linearize(g))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(ctx, g, **kw):
    return ctx.global_ba(g["poses"], g["fixed"], g["points"], g["edge_pose"], g["edge_point"], g["obs"], g["K"], g["huber"], **kw)


def _same(dev, ref):
    for k in FIELDS:
        assert _bits([dev[k]])[0] == _bits([ref[k]])[0] if isinstance(ref[k], float) else dev[k] == ref[k], (k, dev[k], ref[k])
    assert np.array_equal(_bits(dev["poses"]), _bits(ref["poses"]))
    assert np.array_equal(_bits(dev["points"]), _bits(ref["points"]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_equals_the_restatement(ctx, cases, name):
    g, kw, ref, _ = cases[name]
    dev = _run(ctx, g, **kw)
    print("%s: N %d L %d E %d, cost %.6g -> %.6g, status %d, %d LM iterations, %d solves, %d CG iterations, %d capped; device %.6g -> %.6g, "
          "status %d, %d / %d / %d / %d" % (name, len(g["poses"]), len(g["points"]), len(g["obs"]), ref["cost_initial"], ref["cost_final"], ref["status"],
                                            ref["lm_iterations"], ref["n_solves"], ref["cg_iterations_total"], ref["cg_capped"], dev["cost_initial"],
                                            dev["cost_final"], dev["status"], dev["lm_iterations"], dev["n_solves"], dev["cg_iterations_total"],
                                            dev["cg_capped"]))
    _same(dev, ref)
    assert ref["status"] != gb.FAILED
    fx = np.flatnonzero(g["fixed"])
    assert np.array_equal(_bits(dev["poses"][fx]), _bits(np.asarray(g["poses"])[fx]))
    if name == "exact_at_truth":
        assert np.array_equal(_bits(dev["poses"]), _bits(g["poses"])) and np.array_equal(_bits(dev["points"]), _bits(g["points"]))
        assert ref["cost_final"] == 0.0
    else:
        assert ref["cost_final"] < ref["cost_initial"]
    if name == "p48_l600_cap":
        assert ref["cg_capped"] >= 1
    if name == "p4_l300":
        deg = np.bincount(g["edge_pose"])
        assert deg.max() > gb.LANES and deg.max() % 64 != 0 and len(g["points"]) > gb.LANES
    if name == "p3_obs2_obs3":
        assert set(np.bincount(g["edge_point"])) == {2, 3}
    if name == "rejected_trials":                                      # run past convergence: steps that no longer lower the cost are rejected
        assert ref["n_solves"] > ref["lm_iterations"] and ref["status"] == gb.STALLED
    if name == "p24_l400":
        assert int((np.asarray(g["fixed"]) == 0).sum()) > 20


@pytest.mark.parametrize("batch", [1, 64])
def test_no_output_depends_on_the_batch_size(ctx, cases, batch):
    g, kw, ref, _ = cases["p48_l600_cap"]
    _same(_run(ctx, g, cg_batch=batch, **kw), ref)


@pytest.mark.parametrize("name", ["p2_l8", "p4_l300", "huber_outliers", "two_fixed"])
def test_stage_export_equals_the_restatement(ctx, cases, name):
    g, _, _, ref = cases[name]
    dev = ctx.gba_linearize(g["poses"], g["fixed"], g["points"], g["edge_pose"], g["edge_point"], g["obs"], g["K"], g["huber"])
    assert dev["ok"] and ref["ok"]
    for k in ["res", "w", "Jp", "Jl", "Hpp", "bp", "Hll", "bl"]:
        assert np.array_equal(_bits(dev[k]), _bits(ref[k])), k
    assert _bits([dev["cost"]])[0] == _bits([ref["cost"]])[0]


def test_point_behind_a_camera_fails_and_returns_the_input(ctx):
    g = gb.scene(3, 12, 2, seed=24)
    v = g["edge_pose"][np.flatnonzero(g["edge_point"] == 5)[0]]
    g["points"][5] = 1.5 * (-gb.rotation(g["poses"][v][:4]).T @ g["poses"][v][4:])
    dev, ref = _run(ctx, g), gb.optimize(g)
    assert dev["status"] == ref["status"] == gb.FAILED and dev["lm_iterations"] == 0
    _same(dev, ref)
    assert np.array_equal(_bits(dev["poses"]), _bits(g["poses"])) and np.array_equal(_bits(dev["points"]), _bits(g["points"]))
    assert not ctx.gba_linearize(g["poses"], g["fixed"], g["points"], g["edge_pose"], g["edge_point"], g["obs"], g["K"], g["huber"])["ok"]


def test_refusal_through_a_live_context(ctx, hip_lib, cases):
    g = cases["p2_l8"][0]
    ep = np.array(g["edge_pose"]).copy()
    ep[3] = 2                                                          # out of range
    with pytest.raises(hip_lib.YgzHipError) as e:
        ctx.global_ba(g["poses"], g["fixed"], g["points"], ep, g["edge_point"], g["obs"], g["K"], g["huber"])
    assert e.value.code == hip_lib.E_INVALID
    out = _run(ctx, g)                                                 # the context is still good
    assert out["status"] != hip_lib.GBA_FAILED
