"""The stereo bundle adjustment on the MI355X (ygz_hip_stereo_ba / ygz_hip_sba_linearize, ygz_slam_amd/csrc/sba.hip) against its restatement
tests/sba_ref.c, bit for bit: the poses, the points, the outlier flags, every chi2 and every per-round field, on the scenes of
tests/test_sba_ref.py's witness and branch tests and on the sizes where the kernels take another path (1023 / 1024 / 1025 edges, 255 / 256 /
257 points, a pose of 255 / 256 / 257 edges, two poses and eight points); batches of 1 and 64 CG iterations; the stage export; the global
bundle adjustment's own bits on mono level-0 problems without kernel; NULL flag outputs; every refusal through a live context."""
import ctypes as C

import numpy as np
import pytest

import gba_ref as gb
import sba_cases as sc
import sba_ref as sb
from test_gpu_gba import SHAPES

pytestmark = pytest.mark.gpu

INT_FIELDS = ["status", "lm_iterations", "n_solves", "cg_iterations", "cg_capped", "inliers"]
DBL_FIELDS = ["cost_initial", "cost_final", "lambda_"]
ALL = dict(sc.SCENES_D, **sc.SCENES_F, **sc.SCENES_SIZE)


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=4, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """every scene's problem and the restatement's answer, computed once"""
    out = {}
    for name, (make, kw) in ALL.items():
        g = make()
        out[name] = (g, kw, sb.optimize(g, **kw))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _args(g):
    return (g["poses"], g["fixed"], g["points"], g["edge_pose"], g["edge_point"], g["obs"], g["kind"], g["level"], g["K"])


def _run(ctx, g, **kw):
    return ctx.stereo_ba(*_args(g), **sb.call_params(g, **kw))


def _same(dev, ref):
    assert dev["rounds_run"] == ref["rounds_run"]
    for k in INT_FIELDS:
        assert np.array_equal(dev[k], ref[k]), (k, dev[k], ref[k])
    for k in DBL_FIELDS:
        assert np.array_equal(_bits(dev[k]), _bits(ref[k])), (k, dev[k], ref[k])
    assert np.array_equal(_bits(dev["poses"]), _bits(ref["poses"])) and np.array_equal(_bits(dev["points"]), _bits(ref["points"]))
    assert np.array_equal(dev["outlier"], ref["outlier"]) and np.array_equal(_bits(dev["chi2"]), _bits(ref["chi2"]))


@pytest.mark.parametrize("name", list(ALL))
def test_device_equals_the_restatement(ctx, cases, name):
    g, kw, ref = cases[name]
    dev = _run(ctx, g, **kw)
    n = ref["rounds_run"]
    print("%s: N %d L %d E %d, %d rounds, status %s / %s, LM iterations %s / %s, solves %s / %s, inliers %s / %s, cost %s -> %s / %s -> %s"
          % (name, len(g["poses"]), len(g["points"]), len(g["obs"]), n, ref["status"][:n], dev["status"][:n], ref["lm_iterations"][:n],
             dev["lm_iterations"][:n], ref["n_solves"][:n], dev["n_solves"][:n], ref["inliers"][:n], dev["inliers"][:n], ref["cost_initial"][:n],
             ref["cost_final"][:n], dev["cost_initial"][:n], dev["cost_final"][:n]))
    _same(dev, ref)
    n_trials = int(dev["n_solves"].sum())                              # every solve is a trial of at least one batch of the default 8 CG iterations
    assert dev["launches"] >= 5 * n + n_trials * (3 + 3 * 8 + 8) and ref["launches"] == 0
    fx = np.flatnonzero(g["fixed"])
    assert np.array_equal(_bits(dev["poses"][fx]), _bits(np.asarray(g["poses"])[fx]))
    E, L = len(g["obs"]), len(g["points"])
    deg = np.bincount(g["edge_pose"])
    want = {"e1023": E == 1023, "e1024": E == 1024, "e1025": E == 1025, "l255": L == 255, "l256": L == 256, "l257": L == 257,
            "deg255": deg[1] == 255 and not g["fixed"][1], "deg256": deg[1] == 256, "deg257": deg[1] == 257, "p2_l8": (len(g["poses"]), L) == (2, 8)}
    assert want.get(name, True)
    if name == "failed_in_round_0":
        assert dev["status"][0] == sb.FAILED and np.array_equal(_bits(dev["poses"]), _bits(g["poses"]))
        assert np.array_equal(_bits(dev["points"]), _bits(g["points"]))
    elif name != "round_with_no_active_edge":
        assert dev["cost_final"][0] < dev["cost_initial"][0]


@pytest.mark.parametrize("batch", [1, 64])
def test_no_output_depends_on_the_batch_size(ctx, cases, batch):
    g, kw, ref = cases["mono_12x100_outliers"]
    _same(_run(ctx, g, cg_batch=batch, **kw), ref)
    g, kw, ref = cases["capped_cg"]
    _same(_run(ctx, g, cg_batch=batch, **kw), ref)


@pytest.mark.parametrize("name", ["p2_l8", "half_8x80_outliers", "kind_0_among_the_edges", "deg257", "e1025"])
@pytest.mark.parametrize("robust", [0, 1])
def test_stage_export_equals_the_restatement(ctx, cases, name, robust):
    g = cases[name][0]
    dev = ctx.sba_linearize(*_args(g), **sb.call_params(g, robust_rounds=robust))
    ref = sb.linearize(g, robust_rounds=robust)
    assert dev["ok"] and ref["ok"]
    for k in ["res", "w", "Jp", "Jl", "Hpp", "bp", "Hll", "bl"]:
        assert np.array_equal(_bits(dev[k]), _bits(ref[k])), k
    assert _bits([dev["cost"]])[0] == _bits([ref["cost"]])[0]
    base = np.where(g["kind"] != 0, 0.25 ** g["level"], 0.0)
    assert np.array_equal(dev["w"], base) if not robust else np.all(dev["w"] <= base) and (not g["displaced"].any() or (dev["w"] < base).any())


def test_stage_export_of_an_undefined_edge(ctx, cases):
    g = cases["failed_in_round_0"][0]
    dev, ref = ctx.sba_linearize(*_args(g), **sb.call_params(g)), sb.linearize(g)
    assert not dev["ok"] and not ref["ok"]
    for k in ["res", "w", "Jp", "Jl"]:
        assert np.array_equal(_bits(dev[k]), _bits(ref[k])), k


@pytest.mark.parametrize("name", list(SHAPES))
def test_mono_level0_without_kernel_is_the_global_bundle_adjustment(ctx, name):
    """(a) of tests/test_sba_ref.py on the device: ygz_hip_global_ba with huber_delta 0 and ygz_hip_stereo_ba on the same context"""
    make, kw = SHAPES[name]
    g = make()
    old = ctx.global_ba(g["poses"], g["fixed"], g["points"], g["edge_pose"], g["edge_point"], g["obs"], g["K"], 0.0, **kw)
    kw = dict(kw)
    it = kw.pop("max_iterations", 10)
    new = _run(ctx, sb.as_gba(g), rounds=1, robust_rounds=0, iterations=(it,), **kw)
    for a, b in [("status", "status"), ("lm_iterations", "lm_iterations"), ("n_solves", "n_solves"), ("cg_iterations_total", "cg_iterations"),
                 ("cg_capped", "cg_capped")]:
        assert old[a] == new[b][0], (a, old[a], new[b][0])
    for a in ("cost_initial", "cost_final", "lambda_"):
        assert _bits([old[a]])[0] == _bits([new[a][0]])[0], a
    assert np.array_equal(_bits(old["poses"]), _bits(new["poses"])) and np.array_equal(_bits(old["points"]), _bits(new["points"]))


def test_null_flag_outputs(ctx, cases):
    g, kw, ref = cases["half_5x40"]
    dev = ctx.stereo_ba(*_args(g), want_flags=False, **sb.call_params(g, **kw))
    assert dev["outlier"] is None and dev["chi2"] is None
    assert np.array_equal(_bits(dev["poses"]), _bits(ref["poses"])) and np.array_equal(dev["inliers"], ref["inliers"])


def _refused(ctx, hip_lib, g, code=None, **kw):
    with pytest.raises(hip_lib.YgzHipError) as e:
        _run(ctx, g, **kw)
    assert e.value.code == (hip_lib.E_INVALID if code is None else code)


def test_every_refusal_through_a_live_context(ctx, hip_lib, cases):
    g0 = cases["half_5x40"][0]

    def mod(**ch):
        g = dict((k, np.array(v).copy() if isinstance(v, np.ndarray) else v) for k, v in g0.items())
        for k, (i, v) in ch.items():
            g[k][i] = v
        return g
    stereo_e, mono_e = int(np.flatnonzero(g0["kind"] == 2)[0]), int(np.flatnonzero(g0["kind"] == 1)[0])
    _refused(ctx, hip_lib, mod(kind=(3, 3)))
    _refused(ctx, hip_lib, mod(level=(3, 4)))
    _refused(ctx, hip_lib, mod(level=(3, -1)))
    _refused(ctx, hip_lib, mod(obs=((stereo_e, 2), np.nan)))
    _refused(ctx, hip_lib, mod(obs=((mono_e, 1), np.inf)))
    _refused(ctx, hip_lib, mod(edge_pose=(3, 5)))
    _refused(ctx, hip_lib, mod(edge_point=(3, -1)))
    _refused(ctx, hip_lib, mod(poses=((1, 0), np.nan)))
    _refused(ctx, hip_lib, mod(points=((1, 0), np.inf)))
    for kw in (dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=np.inf), dict(chi2_mono=0.0), dict(chi2_stereo=-1.0), dict(chi2_mono=np.nan),
               dict(rounds=0), dict(rounds=5), dict(robust_rounds=-1), dict(robust_rounds=5), dict(iterations=(5, 0)), dict(iterations=(1001, 10)),
               dict(rounds=3), dict(max_trials=0), dict(cg_tol=1.0), dict(cg_batch=1025)):
        _refused(ctx, hip_lib, g0, **kw)
    # the degree rules count present edges only: a point left with one present edge, a free pose left with none
    l = int(g0["edge_point"][0])
    g = mod()
    g["kind"][np.flatnonzero(g["edge_point"] == l)[1:]] = 0
    _refused(ctx, hip_lib, g)
    g = mod()
    g["kind"][g["edge_pose"] == 2] = 0
    _refused(ctx, hip_lib, g)
    g = mod()
    g["fixed"][:] = 1
    _refused(ctx, hip_lib, g)
    # what is never read is never refused: uR of a mono edge, the baseline without a stereo edge, an unused iterations entry
    ok = _run(ctx, mod(obs=((mono_e, 2), np.nan)))
    assert ok["status"][0] != sb.FAILED
    g = mod()
    g["kind"][:] = 1
    assert _run(ctx, g, baseline=0.0)["status"][0] != sb.FAILED
    assert _run(ctx, g0, rounds=1, iterations=(5, -7, 0, 0))["rounds_run"] == 1
    _same(_run(ctx, g0, **cases["half_5x40"][1]), cases["half_5x40"][2])          # the context is still good


def test_two_level_context_rejects_level_2(hip_lib, cases):
    g = cases["p2_l8"][0]
    c = hip_lib.HipContext(width=34, height=32, levels=2, max_frames=2)
    try:
        assert set(g["level"]) == {0, 1, 2, 3}
        with pytest.raises(hip_lib.YgzHipError) as e:
            _run(c, g)
        assert e.value.code == hip_lib.E_INVALID
        low = dict(g, level=np.minimum(g["level"], 1))
        _same(_run(c, low), sb.optimize(low))
    finally:
        c.close()
