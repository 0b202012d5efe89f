"""The local-map fusion search on the MI355X (ygz_slam_amd/csrc/lfuse.hip: k_lfuse_search) against the restatement tests/lfuse_ref.c: every
output EQUAL, bit for bit.

Shapes: n_pt in {1, 63, 64, 65, 255, 256, 257} (a block is 256 points, a wavefront 64: one lane, one short of a wavefront, exactly one, one
more, one short of a block, one block, one more) and n_kp in {1, 255, 256, 257, 513, 768} (a tile is 256 keypoints: one entry, one short of
a tile, one tile, one more, two and a ragged third, three full ones); 1, 3 and 64 problems on one shared set; two sets of different sizes
read by interleaved problems; a set with no points; all-mono with kp_ur NULL, all-stereo and mixed; with and without pt_normal, kp_taken and
pt_skip; the decoy scene; other parameters; the projection search's results with the gate open; YGZ_E_CAPACITY one above each limit and the
validation errors through a live context; a second identical call."""
import numpy as np
import pytest

import lfuse_ref as lf
import proj_ref as pr
from conftest import make_ctx
from test_lfuse_ref import DECOY_THRESHOLD, decoy_rates

pytestmark = pytest.mark.gpu

NAMES = ("match", "dist", "pred_level", "reason", "n_gated", "counts")
N_PT = [1, 63, 64, 65, 255, 256, 257]
N_KP = [1, 255, 256, 257, 513, 768]
K4 = lf.K4_DEFAULT


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=2, intrinsics=K4)
    yield c
    c.close()


def check(ctx, sets, problems, **fields):
    got = ctx.local_fuse_search(sets, problems, K4, **fields)
    want = lf.search(sets, problems, K4, 640, 480, 3, **fields)
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(got["offsets"], lf.offsets(sets, problems))
    return got


@pytest.mark.parametrize("n_pt", N_PT)
def test_every_point_count(ctx, n_pt):
    seen = 0
    for n_kp in N_KP:
        s, p = lf.split(lf.scene(n_pt, n_kp, 1000 + 7 * n_pt + n_kp, taken=n_kp % 2 == 0, skip=n_pt > 1, normals=n_kp != 513))
        got = check(ctx, [s], [p])
        seen += int((got["match"] >= 0).sum())
    assert seen > 0 or n_pt == 1


@pytest.mark.parametrize("n_problems", [1, 3, 64])
def test_problems_on_one_shared_set(ctx, n_problems):
    sets, pbs = lf.shared_scene(257, 300 if n_problems < 64 else 130, n_problems, 40 + n_problems, taken=True, skip=True)
    got = check(ctx, sets, pbs)
    assert got["counts"].shape == (n_problems, 2) and (got["counts"][:, 0] > 0).all() and got["n_gated"].sum() > 0
    again = ctx.local_fuse_search(sets, pbs, K4)                       # a second identical call gives identical bytes
    for k in NAMES:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_two_sets_interleaved_and_an_empty_set(ctx):
    a, pa = lf.shared_scene(65, 257, 3, 31)
    b, pb = lf.shared_scene(513, 255, 2, 32, normals=False)
    empty = dict(pw=np.zeros((0, 3)), pt_desc=np.zeros((0, 32), np.uint8), pt_dmax=np.zeros(0))
    sets = [a[0], empty, b[0]]
    pbs = [dict(pa[0], set=0), dict(pb[0], set=2), dict(pa[1], set=1, pt_skip=None), dict(pa[1], set=0), dict(pb[1], set=2), dict(pa[2], set=0)]
    got = check(ctx, sets, pbs)
    assert list(got["offsets"]) == [0, 65, 578, 578, 643, 1156, 1221] and (got["counts"][2] == 0).all()
    assert (got["counts"][[0, 1, 3, 4, 5], 0] > 0).all()
    # every problem reads the empty set: nothing to do, no launch
    got = check(ctx, sets, [dict(pa[0], set=1)])
    assert len(got["match"]) == 0


def test_mono_stereo_and_mixed(ctx):
    sets, pbs = lf.shared_scene(257, 513, 1, 51)
    p = pbs[0]
    mono = {k: v for k, v in p.items() if k != "kp_ur"}                 # kp_ur NULL
    g0 = check(ctx, sets, [mono])
    g1 = check(ctx, sets, [dict(p, kp_ur=np.full(513, -1.0))])
    assert g0["match"].tobytes() == g1["match"].tobytes()
    _, ps = lf.shared_scene(257, 513, 1, 51, stereo=1.0)
    assert (ps[0]["kp_ur"] >= 0).mean() > 0.9
    g2 = check(ctx, sets, [dict(ps[0], kp_ur=np.maximum(ps[0]["kp_ur"], 0.0))])    # every keypoint stereo
    g3 = check(ctx, sets, [p])
    assert (p["kp_ur"] >= 0).any() and (p["kp_ur"] < 0).any()
    assert g2["n_gated"].sum() > 0 and g3["n_gated"].sum() > 0 and g2["match"].tobytes() != g0["match"].tobytes()


def test_decoy_scene_and_other_parameters(ctx):
    mono, stereo = decoy_rates(lambda s, p: check(ctx, s, p))
    assert stereo < DECOY_THRESHOLD < mono
    sets, pbs = lf.shared_scene(255, 257, 2, 61, baseline=0.25)
    check(ctx, sets, pbs, th=5.0, th_dist=70, baseline=0.25, chi2_mono=3.0, chi2_stereo=20.0)
    check(ctx, sets, pbs, th=1.5, th_dist=0)
    check(ctx, sets, pbs, th_dist=256, chi2_mono=1e300, chi2_stereo=1e300)


def test_open_gate_is_the_projection_search_on_the_device(ctx):
    pbs, sets, lp = [], [], []
    for q, (n_pt, n_kp) in enumerate([(257, 300), (64, 768), (300, 513)]):
        sc = pr.scene(n_pt, n_kp, 70 + q, taken=q == 1, skip=q != 1)
        s, p = lf.split(sc, q)
        pbs.append(sc); sets.append(s); lp.append(p)
    for th in (3.0, 10.0):
        got = ctx.local_fuse_search(sets, lp, K4, th=th, chi2_mono=1e300, chi2_stereo=1e300)
        dev = ctx.search_by_projection(pbs, K4, th=th, th_dist=50, claim=0)
        ref = pr.search(pbs, K4, th=th, th_dist=50, claim=0)
        for k in ("match", "dist", "pred_level"):
            assert np.array_equal(got[k], dev[k]) and np.array_equal(got[k], ref[k]), (th, k)
        assert (got["match"] >= 0).sum() > 0 and (got["n_gated"] == 0).all()


def test_capacity_and_validation_through_a_live_context(ctx, hip_lib):
    E = hip_lib.YgzHipError
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    sets, pbs = lf.shared_scene(20, 30, 1, 81)
    s, p = sets[0], pbs[0]

    def rc(fn):
        with pytest.raises(E) as e:
            fn()
        return e.value.code
    assert rc(lambda: ctx.local_fuse_search([s], [p] * (hip_lib.LFUSE_MAX_PROBLEMS + 1), K4)) == CAP
    assert rc(lambda: ctx.local_fuse_search([s] * (hip_lib.LFUSE_MAX_SETS + 1), [p], K4)) == CAP
    n = hip_lib.LFUSE_MAX_PAIRS // 2 + 1
    big = dict(pw=np.ones((n, 3)), pt_desc=np.zeros((n, 32), np.uint8), pt_dmax=np.ones(n))
    q = {k: v for k, v in p.items() if k != "pt_skip"}
    assert rc(lambda: ctx.local_fuse_search([big], [q, q], K4)) == CAP
    m = ctx.cells + 1
    wide = dict(T=p["T"], kp_px=np.zeros((m, 2)), kp_level=np.zeros(m, np.int32), kp_desc=np.zeros((m, 32), np.uint8))
    assert rc(lambda: ctx.local_fuse_search([s], [wide], K4)) == CAP
    assert rc(lambda: ctx.local_fuse_search([s], [], K4)) == INV and rc(lambda: ctx.local_fuse_search([], [p], K4)) == INV
    assert rc(lambda: ctx.local_fuse_search([s], [dict(p, set=1)], K4)) == INV and rc(lambda: ctx.local_fuse_search([s], [dict(p, set=-1)], K4)) == INV
    assert rc(lambda: ctx.local_fuse_search([s], [dict(p, kp_level=np.full(30, 3))], K4)) == INV           # outside the 3-level pyramid
    assert rc(lambda: ctx.local_fuse_search([s], [dict(p, kp_level=np.full(30, -1))], K4)) == INV
    assert rc(lambda: ctx.local_fuse_search([s], [dict(p, kp_ur=np.full(30, np.nan))], K4)) == INV
    assert rc(lambda: ctx.local_fuse_search([s], [dict(p, T=[0, 0, 0, np.inf, 0, 0, 0])], K4)) == INV
    assert rc(lambda: ctx.local_fuse_search([dict(s, pw=np.full((20, 3), np.nan))], [p], K4)) == INV
    assert rc(lambda: ctx.local_fuse_search([dict(s, pt_dmax=np.full(20, np.inf))], [p], K4)) == INV
    assert rc(lambda: ctx.local_fuse_search([s], [p], (0.0, 1.0, 1.0, 1.0))) == INV
    for bad in (dict(th=0.0), dict(th=float("inf")), dict(th_dist=-1), dict(th_dist=257), dict(baseline=0.0), dict(chi2_mono=0.0),
                dict(chi2_stereo=-1.0), dict(chi2_mono=float("nan"))):
        assert rc(lambda: ctx.local_fuse_search([s], [p], K4, **bad)) == INV, bad
    check(ctx, [s], [p])                                               # the context still works after the refusals
