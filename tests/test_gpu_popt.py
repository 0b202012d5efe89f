"""ygz_hip_optimize_pose_stereo on the MI355X against the restatement tests/popt_ref.c: every output of every frame and edge equal, doubles bit
for bit -- pose, per-round cost / lambda / iterations / status, chi2, flags and counts -- on the scenes a .. r of tests/popt_ref.py with their
parameters and with the plain defaults (min_rel_decrease = 0, where the rounds run down to the rounding floor of the cost); a call of many frames
equal to the same frames sent one per call; NULL optional outputs; n_frames = 0; every validation error through a live context; a 34 x 32 context
with 2 levels rejects level 2.  One context for the module."""
import ctypes

import numpy as np
import pytest

import popt_ref as pr

pytestmark = pytest.mark.gpu

KEYS = ("pose", "outlier", "chi2", "inliers", "rounds_run", "status", "lm_iterations", "cost_initial", "cost_final", "lambda")


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=pr.WIDTH, height=pr.HEIGHT, levels=pr.LEVELS, max_frames=2)
    yield c
    c.close()


def to_abi(hip_lib, p):
    return hip_lib.PoseOptParams(*[getattr(p, n) for n, _ in pr.Params._fields_])


def run(ctx, hip_lib, frames, p, **kw):
    a = pr.pack(frames)
    return ctx.optimize_pose_stereo(a["frame_off"], a["pw"], a["obs"], a["level"], a["kind"], a["poses"], params=to_abi(hip_lib, p), **kw)


_want = {}


def want(frames, p):
    """the restatement's outputs of the frames in the call's layout; computed once per (frames, parameters)"""
    key = (tuple(id(f) for f in frames), tuple(pr.fields(p).values()))
    if key not in _want:
        rs = [pr.optimize(f, p) for f in frames]
        w = {k: np.stack([r[k] for r in rs]) for k in ("pose", "status", "lm_iterations", "cost_initial", "cost_final", "lambda")}
        w["outlier"] = np.concatenate([r["outlier"] for r in rs])
        w["chi2"] = np.concatenate([r["chi2"] for r in rs])
        w["inliers"] = np.array([r["inliers"] for r in rs], np.int32)
        w["rounds_run"] = np.array([r["rounds_run"] for r in rs], np.int32)
        _want[key] = (frames, w)
    return _want[key][1]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_equal(got, w, what):
    for k in KEYS:
        assert got[k].shape == w[k].shape and got[k].dtype == w[k].dtype, (what, k, got[k].shape, w[k].shape)
        if not np.array_equal(bits(got[k]), bits(w[k])):
            bad = np.argwhere(bits(got[k]) != bits(w[k]))
            first = tuple(bad[0])
            raise AssertionError("%s: %s differs in %d places, first at %s: device %r, restatement %r" % (what, k, len(bad), first, got[k][first], w[k][first]))


@pytest.mark.parametrize("variant", ["scene", "defaults"])
@pytest.mark.parametrize("name", pr.SCENES)
def test_every_output_is_the_restatements(ctx, hip_lib, name, variant):
    frames, p = pr.scene(name)
    if variant == "defaults":
        p = pr.params(**dict(pr.fields(p), min_rel_decrease=0.0))
    got = run(ctx, hip_lib, frames, p)
    assert_equal(got, want(frames, p), "%s/%s" % (name, variant))


def test_frames_of_a_call_equal_single_calls(ctx, hip_lib):
    p = pr.params()
    for frames in (pr.scene("j")[0], pr.mixed_call(64)):
        got = run(ctx, hip_lib, frames, p)
        assert_equal(got, want(frames, p), "call of %d frames" % len(frames))
        off = pr.pack(frames)["frame_off"]
        for q in (0, 1, len(frames) // 2, len(frames) - 1):
            one = run(ctx, hip_lib, [frames[q]], p)
            for k in ("pose", "inliers", "rounds_run", "status", "lm_iterations", "cost_initial", "cost_final", "lambda"):
                assert np.array_equal(bits(one[k][0]), bits(got[k][q])), (q, k)
            for k in ("outlier", "chi2"):
                assert np.array_equal(bits(one[k]), bits(got[k][off[q]:off[q + 1]])), (q, k)


def test_null_outputs_empty_call_and_empty_frames(ctx, hip_lib):
    frames, p = pr.scene("c")
    got = run(ctx, hip_lib, frames, p, outputs=False)
    assert sorted(got) == ["pose"] and np.array_equal(bits(got["pose"]), bits(want(frames, p)["pose"]))
    none = run(ctx, hip_lib, [], p)
    assert none["pose"].shape == (0, 7) and none["inliers"].shape == (0,)
    # a frame without edges between two with: FAILED in round 0, its pose untouched bit for bit
    empty = pr.Frame(np.zeros((0, 3)), np.zeros((0, 3)), [], [], frames[0].pose)
    trio = [frames[0], empty, pr.scene("a")[0][0]]
    got = run(ctx, hip_lib, trio, p)
    assert_equal(got, want(trio, p), "empty frame")
    assert got["rounds_run"][1] == 1 and got["status"][1, 0] == hip_lib.POPT_FAILED and got["inliers"][1] == 0
    assert np.array_equal(bits(got["pose"][1]), bits(empty.pose))
    for name in ("f", "g"):
        fr = pr.scene(name)[0][0]
        got = run(ctx, hip_lib, [fr], p)
        assert got["status"][0, 0] == hip_lib.POPT_FAILED and np.array_equal(bits(got["pose"][0]), bits(fr.pose)), name


def _raw(c, hip_lib, a, p, n_frames=None, **over):
    """the C call with any argument replaced; returns the code"""
    lib = c.lib
    hip_lib.popt_argtypes(lib)
    ip, dp, bp = (lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), (lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))), \
        (lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    poses = a["poses"].copy()
    args = dict(ctx=c._ctx, n_frames=len(a["frame_off"]) - 1 if n_frames is None else n_frames, frame_off=ip(a["frame_off"]), pw=dp(a["pw"]),
                obs=dp(a["obs"]), level=ip(a["level"]), kind=bp(a["kind"]), params=ctypes.byref(p) if p is not None else None, poses=dp(poses))
    args.update(over)
    rc = lib.ygz_hip_optimize_pose_stereo(args["ctx"], args["n_frames"], args["frame_off"], args["pw"], args["obs"], args["level"], args["kind"],
                                          args["params"], args["poses"], *(None,) * 9)
    assert np.array_equal(bits(poses), bits(a["poses"])) or rc == hip_lib.OK       # a refused call writes nothing
    return rc


def test_every_validation_error(ctx, hip_lib):
    frames, p0 = pr.scene("c")
    a = pr.pack(frames + pr.scene("a")[0])
    INV, OK = hip_lib.E_INVALID, hip_lib.OK
    P = lambda **kw: to_abi(hip_lib, pr.params(**kw))
    assert _raw(ctx, hip_lib, a, P()) == OK
    assert _raw(ctx, hip_lib, a, None) == INV
    assert _raw(ctx, hip_lib, a, P(), ctx=None) == INV
    for key in ("frame_off", "pw", "obs", "level", "kind", "poses"):
        assert _raw(ctx, hip_lib, a, P(), **{key: None}) == INV, key
    assert _raw(ctx, hip_lib, a, P(), n_frames=-1) == INV
    for off in ([1, 300, 600], [0, 400, 300]):
        b = dict(a, frame_off=np.array(off, np.int32))
        assert _raw(ctx, hip_lib, b, P()) == INV, off
    kind = a["kind"].copy()
    kind[17] = 3
    assert _raw(ctx, hip_lib, dict(a, kind=kind), P()) == INV
    for lv in (-1, pr.LEVELS):
        level = a["level"].copy()
        level[5] = lv
        assert _raw(ctx, hip_lib, dict(a, level=level), P()) == INV, lv
    nan, inf = float("nan"), float("inf")
    for bad in (dict(baseline=nan), dict(baseline=inf), dict(baseline=0.0), dict(baseline=-0.1), dict(chi2_mono=0.0), dict(chi2_mono=-1.0),
                dict(chi2_mono=nan), dict(chi2_stereo=0.0), dict(chi2_stereo=inf), dict(min_rel_decrease=nan), dict(rounds=0), dict(rounds=9),
                dict(iterations=0), dict(iterations=65), dict(max_trials=0), dict(max_trials=65)):
        assert _raw(ctx, hip_lib, a, P(**bad)) == INV, bad
    # without a stereo edge the baseline is not looked at
    mono = pr.pack(pr.scene("b")[0])
    assert _raw(ctx, hip_lib, mono, P(baseline=0.0)) == OK
    assert _raw(ctx, hip_lib, a, P(), n_frames=0) == OK


def test_a_small_context_rejects_a_level_outside_its_pyramid(hip_lib):
    c = hip_lib.HipContext(width=34, height=32, levels=2, max_frames=1)
    try:
        fr = pr.scene("j")[0][2]
        p = to_abi(hip_lib, pr.params())
        assert fr.level.max() == 3
        assert _raw(c, hip_lib, pr.pack([fr]), p) == hip_lib.E_INVALID
        low = pr.pack([fr.replace(level=fr.level % 2)])
        assert _raw(c, hip_lib, low, p) == hip_lib.OK
    finally:
        c.close()
