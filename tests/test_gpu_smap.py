"""Stereo map-point creation on the MI355X (ygz_slam_amd/csrc/smap.hip: k_smap_pairs, k_smap_keyframe) against the restatement
tests/smap_ref.c: every output EQUAL, the doubles bit for bit.

Pairs: the four scenes at 0, 1, 63, 64, 65 and 257 pairs per problem (one workgroup is 64 lanes: an idle workgroup's worth, one lane, one
short of a workgroup, exactly one, one more, several with a ragged end), 1, 3 and 32 problems per call (the 32 mix every size, empty ones
included, so that workgroups straddle problems and the table's lookup skips empty entries), all-mono and all-stereo problems, the two
hand-made pairs for the codes 2 and 7, a second identical call, YGZ_E_CAPACITY one above each limit and the validation errors through a
live context.  Keyframe points: n = 1, 64, 65, 1000 and ygz_hip_max_keypoints of a 320 x 240 context (768: three tiles of 256 depths, the
1000 on a 640 x 480 one: a ragged fourth tile), the (n_depth, c) grid of the CPU test, n_depth = 0."""
import numpy as np
import pytest

import smap_ref as sm
from conftest import make_ctx

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = make_ctx(hip_lib, width=320, height=240, levels=3, max_frames=2, intrinsics=sm.K4)
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def restate(problems, K4=sm.K4, params=None):
    out = [sm.create(pb, K4, params) for pb in problems]
    code = np.concatenate([o[0] for o in out]) if out else np.zeros(0, np.int32)
    method = np.concatenate([o[1] for o in out])
    pos = np.concatenate([o[2] for o in out])
    counts = np.array([[int((o[0] == 0).sum()), int(((o[0] == 0) & (o[1] == 1)).sum())] for o in out], np.int32)
    return code, method, pos, counts


def check(ctx, problems, K4=sm.K4, params=None, fields=None):
    fields = fields or {}
    got = ctx.stereo_create_map_points(problems, K4, **fields)
    p = params if params is not None else sm.default_params(**fields)
    code, method, pos, counts = restate(problems, K4, p)
    assert np.array_equal(got["code"], code) and np.array_equal(got["method"], method)
    assert same_bits(got["pos_world"], pos)
    assert np.array_equal(got["counts"], counts)
    return got


@pytest.mark.parametrize("kind", sm.SCENE_KINDS)
def test_one_problem_at_every_size(ctx, kind):
    seen = np.zeros(9, np.int64)
    for n in SIZES:
        got = check(ctx, [sm.scene(kind, n, 300 + n)])
        assert len(got["code"]) == n
        seen += np.bincount(got["code"], minlength=9)
    assert seen[0] > 0


def test_three_problems(ctx):
    pbs = [sm.scene("forward", 65, 41), sm.scene("wrong", 63, 42), sm.scene("sideways", 257, 43)]
    got = check(ctx, pbs)
    assert list(got["offsets"]) == [0, 65, 128, 385]
    assert len(set(np.unique(got["method"]))) == 4 and len(np.unique(got["code"])) >= 7


def test_32_problems_of_mixed_sizes(ctx):
    sizes = [0, 1, 63, 0, 64, 65, 257, 0] * 4
    pbs = [sm.scene(sm.SCENE_KINDS[q % 4], n, 500 + q) for q, n in enumerate(sizes)]
    got = check(ctx, pbs)
    assert len(got["code"]) == sum(sizes) and got["counts"].shape == (32, 2) and np.all(got["counts"][np.array(sizes) == 0] == 0)
    # a second identical call gives identical bytes
    again = ctx.stereo_create_map_points(pbs, sm.K4)
    for k in ("code", "method", "pos_world", "counts"):
        assert same_bits(got[k], again[k]), k


def test_all_mono_and_all_stereo(ctx):
    mono = sm.scene("mono", 257, 61)
    assert (mono["ur1"] < 0).all() and (mono["ur2"] < 0).all()
    no_depth = dict(mono, depth1=None, depth2=None)                   # the depths of a problem without a stereo side may be absent
    got = ctx.stereo_create_map_points([no_depth], sm.K4)
    code, method, pos, _ = restate([mono])
    assert np.array_equal(got["code"], code) and np.array_equal(got["method"], method) and same_bits(got["pos_world"], pos)
    assert set(np.unique(method)) <= {0, 1}
    stereo = sm.scene("forward", 300, 62, mono_share=0.0)            # a measurement left of the picture is mono: keep 257 pairs that are not
    stereo = sm.subset(stereo, np.flatnonzero((stereo["ur1"] >= 0) & (stereo["ur2"] >= 0))[:257])
    assert stereo["n"] == 257
    assert (stereo["ur1"] >= 0).all() and (stereo["ur2"] >= 0).all()
    got = check(ctx, [stereo, mono])
    assert not (got["method"][:257] == 3).any()                       # side 2 is asked only when side 1 is not stereo


def test_hand_made_codes_and_other_parameters(ctx):
    for pb, K4, p, want_code, want_method in sm.edge_cases():
        got = ctx.stereo_create_map_points([pb], K4, params=ctx.default_smap_params(cos_parallax_max=p.cos_parallax_max))
        assert got["code"][0] == want_code and got["method"][0] == want_method and np.all(got["pos_world"] == 0.0)
    fields = dict(baseline=0.25, chi2_mono=3.0, chi2_stereo=4.5, cos_parallax_max=0.99999, ratio_factor=2.5)
    check(ctx, [sm.scene("forward", 257, 71, baseline=0.25), sm.scene("wrong", 65, 72, baseline=0.25)], fields=fields)


def kf_check(ctx, T, px, depth, has, fields=None):
    fields = fields or {}
    got = ctx.stereo_keyframe_points(T, px, depth, has, sm.K4, **fields)
    want = sm.keyframe_points(T, px, depth, has, sm.K4, sm.default_params(**fields))
    assert np.array_equal(got["rank"], want["rank"]) and np.array_equal(got["selected"], want["selected"])
    assert same_bits(got["pos_world"], want["pos_world"])
    assert (got["n_depth"], got["n_close"], got["n_selected"]) == (want["n_depth"], want["n_close"], int(want["selected"].sum()))
    return got


def test_keyframe_points_at_every_size(ctx, hip_lib):
    assert ctx.cells == 768
    for n in (1, 64, 65, ctx.cells):
        nd = n - n // 5
        T, px, depth, has = sm.keyframe_scene(n, nd, nd // 3, 800 + n)
        got = kf_check(ctx, T, px, depth, has)
        assert got["n_depth"] == nd
    big = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=2, intrinsics=sm.K4)
    try:
        T, px, depth, has = sm.keyframe_scene(1000, 900, 400, 77)
        got = kf_check(big, T, px, depth, has)
        assert got["n_close"] == 400 and (got["rank"] >= 0).sum() == 401
        again = big.stereo_keyframe_points(T, px, depth, has, sm.K4)
        for k in ("rank", "selected", "pos_world"):
            assert same_bits(got[k], again[k]), k
    finally:
        big.close()


@pytest.mark.parametrize("n_depth,c", sm.KEYFRAME_GRID)
def test_keyframe_grid(ctx, n_depth, c):
    T, px, depth, has = sm.keyframe_scene(n_depth + 37, n_depth, c, 100 + 7 * n_depth + c)
    got = kf_check(ctx, T, px, depth, has)
    assert (got["n_depth"], got["n_close"]) == (n_depth, c)
    if n_depth == 0:
        assert not got["selected"].any() and np.all(got["rank"] == -1) and np.all(got["pos_world"] == 0.0)
    kf_check(ctx, T, px, depth, has, fields=dict(th_depth=5.0, min_close=7))


def test_capacity_and_validation_through_a_live_context(ctx, hip_lib):
    E = hip_lib.YgzHipError
    one = sm.scene("forward", 4, 5)

    def rc(fn):
        with pytest.raises(E) as e:
            fn()
        return e.value.code
    assert rc(lambda: ctx.stereo_create_map_points([one] * (hip_lib.SMAP_MAX_PROBLEMS + 1), sm.K4)) == hip_lib.E_CAPACITY
    big = sm.scene("sideways", hip_lib.SMAP_MAX_PAIRS // 2 + 1, 6)
    assert rc(lambda: ctx.stereo_create_map_points([big, big], sm.K4)) == hip_lib.E_CAPACITY
    T, px, depth, has = sm.keyframe_scene(ctx.cells + 1, 10, 5, 7)
    assert rc(lambda: ctx.stereo_keyframe_points(T, px, depth, has, sm.K4)) == hip_lib.E_CAPACITY
    INV = hip_lib.E_INVALID
    assert rc(lambda: ctx.stereo_create_map_points([], sm.K4)) == INV
    assert rc(lambda: ctx.stereo_create_map_points([dict(one, level1=np.full(4, 3))], sm.K4)) == INV          # outside the 3-level pyramid
    assert rc(lambda: ctx.stereo_create_map_points([dict(one, level2=np.full(4, -1))], sm.K4)) == INV
    assert rc(lambda: ctx.stereo_create_map_points([dict(one, px1=np.full((4, 2), np.nan))], sm.K4)) == INV
    bad_depth = dict(one, ur1=np.full(4, 10.0), depth1=np.full(4, np.inf))
    assert rc(lambda: ctx.stereo_create_map_points([bad_depth], sm.K4)) == INV
    assert rc(lambda: ctx.stereo_create_map_points([dict(one, ur1=np.full(4, 10.0), depth1=None)], sm.K4)) == INV
    assert rc(lambda: ctx.stereo_create_map_points([dict(one, T2=[0, 0, 0, np.nan, 0, 0, 0])], sm.K4)) == INV
    assert rc(lambda: ctx.stereo_create_map_points([one], (0.0, 1.0, 1.0, 1.0))) == INV
    for bad in (dict(baseline=0.0), dict(chi2_mono=-1.0), dict(chi2_stereo=0.0), dict(cos_parallax_max=0.0), dict(ratio_factor=0.5),
                dict(th_depth=0.0), dict(min_close=-1), dict(baseline=float("nan"))):
        assert rc(lambda: ctx.stereo_create_map_points([one], sm.K4, **bad)) == INV, bad
        assert rc(lambda: ctx.stereo_keyframe_points(T[:7], px[:3], depth[:3], has[:3], sm.K4, **bad)) == INV, bad
    assert rc(lambda: ctx.stereo_keyframe_points(T, px[:3], [1.0, np.nan, 2.0], has[:3], sm.K4)) == INV
    # a mono side's depth is never read: garbage there changes nothing
    garbage = dict(one, ur1=np.full(4, -1.0), depth1=np.full(4, np.nan))
    check(ctx, [garbage])
    # the context still works after the refusals
    check(ctx, [one])
