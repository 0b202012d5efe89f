"""The stereo tracking search on the MI355X (ygz_slam_amd/csrc/strack.hip: k_strack_search and the host walk of its entry point) against the
restatement tests/strack_ref.c: every output EQUAL, bit for bit.

Shapes: n_pt in {1, 63, 64, 65, 255, 256, 257} (a block is 256 points, a wavefront 64) times n_kp in {1, 7, 8, 9, 255, 256, 257, 513} (the
sweep tests eight tile entries at a time, a tile is 256 keypoints); every shape as ONE call of four problems over two sets: FRAME with
direction -1, 0 and +1, and LOCAL; pyramids of 1 and 3 levels; 1, 3 and 64 problems with the modes mixed; the crafted scenes of
tests/test_strack_ref.py (contention, overflow, ratio, orientation, decoys); an empty set; kp_ur NULL; sets without angles; other parameters;
YGZ_E_CAPACITY one above each limit and the validation errors through a live context; a second identical call."""
import numpy as np
import pytest

import strack_ref as st
from conftest import make_ctx

pytestmark = pytest.mark.gpu

NAMES = ("match", "dist", "level", "reason", "outcome", "n_cand", "n_gated", "proj", "cand", "counts", "rot")
N_PT = [1, 63, 64, 65, 255, 256, 257]
N_KP = [1, 7, 8, 9, 255, 256, 257, 513]
K4 = st.K4_DEFAULT


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=2, intrinsics=K4)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx1(hip_lib):
    c = make_ctx(hip_lib, width=640, height=480, levels=1, max_frames=2, intrinsics=K4)
    yield c
    c.close()


def check(ctx, sets, problems, L=3, **fields):
    got = ctx.stereo_track_search(sets, problems, K4, **fields)
    want = st.search(sets, problems, K4, 640, 480, L, **fields)
    for k in NAMES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert np.array_equal(got["offsets"], st.offsets(sets, problems))
    return got


def four(n_pt, n_kp, seed, L=3):
    """FRAME with the three directions and LOCAL, over two sets"""
    fs, fp = st.frame_scene(n_pt, n_kp, seed, L=L, taken=n_kp % 2 == 0, skip=n_pt > 1)
    ls, lp = st.local_scene(n_pt, n_kp, seed + 1, L=L, taken=n_kp % 2 == 1, skip=n_pt > 1)
    return [fs[0], ls[0]], [dict(fp[0], direction=-1), dict(fp[0], direction=0), dict(fp[0], direction=1), dict(lp[0], set=1)]


@pytest.mark.parametrize("n_pt", N_PT)
def test_every_point_count(ctx, n_pt):
    seen = np.zeros(4, np.int64)
    for n_kp in N_KP:
        sets, pbs = four(n_pt, n_kp, 2000 + 7 * n_pt + n_kp)
        got = check(ctx, sets, pbs)
        seen += got["counts"][:, 0]
    assert (seen > 0).all() or n_pt == 1


@pytest.mark.parametrize("n_pt,n_kp", [(65, 9), (257, 257), (256, 513)])
def test_one_level_pyramid(ctx1, n_pt, n_kp):
    sets, pbs = four(n_pt, n_kp, 3000 + n_pt + n_kp, L=1)
    got = check(ctx1, sets, pbs, L=1)
    assert (got["counts"][:, 0] > 0).all()


@pytest.mark.parametrize("n_problems", [1, 3, 64])
def test_problems_with_the_modes_mixed(ctx, n_problems):
    sets, pbs = st.mixed_scene(n_problems, 257, 300 if n_problems < 64 else 130, 40 + n_problems)
    got = check(ctx, sets, pbs)
    assert got["counts"].shape == (n_problems, 4) and (got["counts"][:, 0] > 0).all() and got["n_gated"].sum() > 0
    again = ctx.stereo_track_search(sets, pbs, K4)                     # a second identical call gives identical bytes
    for k in NAMES:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_crafted_scenes(ctx):
    for mode in (st.FRAME, st.LOCAL):
        got = check(ctx, *st.contention_scene(1, mode))
        assert (got["outcome"] == st.NO_CANDIDATE).any()
        got = check(ctx, *st.overflow_scene(2, mode))
        assert got["counts"][0, 2] == 40 and (got["n_cand"] > st.TOPK).all()
    got = check(ctx, *st.ratio_scene(3))
    assert (got["outcome"] == st.RATIO).any()
    got = check(ctx, *st.frame_scene(513, 768, 3))
    assert got["counts"][0, 3] > 0 and (got["outcome"] == st.ORIENTATION).sum() == got["counts"][0, 3]
    off = check(ctx, *st.frame_scene(513, 768, 3), check_orientation=0)
    assert off["counts"][0, 3] == 0 and off["counts"][0, 0] == got["counts"][0, 0] + got["counts"][0, 3]


def test_decoys_fall_to_the_right_column(ctx):
    n = min(2000, ctx.cells // 2)                                      # two keypoints per point, within ygz_hip_max_keypoints
    assert n >= 500
    got = check(ctx, *st.decoy_scene(n, 9, with_columns=False))
    assert np.array_equal(got["match"], np.arange(n))
    got = check(ctx, *st.decoy_scene(n, 9, with_columns=True))
    assert np.array_equal(got["match"], np.arange(n) + n) and (got["n_gated"] > 0).all()


def test_empty_set_null_columns_no_angles_and_other_parameters(ctx):
    fs, fp = st.frame_scene(257, 513, 51)
    ls, lp = st.local_scene(255, 257, 52, taken=True, skip=True)
    empty = dict(pw=np.zeros((0, 3)), pt_desc=np.zeros((0, 32), np.uint8), pt_level=np.zeros(0, np.int32), pt_dmax=np.zeros(0),
                 pt_normal=np.zeros((0, 3)))
    sets = [fs[0], empty, ls[0]]
    pbs = [dict(fp[0], set=0), dict(lp[0], set=2), dict(fp[0], set=1, pt_skip=None), dict(lp[0], set=1, pt_skip=None), dict(fp[0], set=0, direction=1)]
    got = check(ctx, sets, pbs)
    assert list(got["offsets"]) == [0, 257, 512, 512, 512, 769] and (got["counts"][2:4] == 0).all()
    got = check(ctx, sets, [dict(fp[0], set=1, pt_skip=None)])                   # every problem reads the empty set: nothing to do, no launch
    assert len(got["match"]) == 0 and (got["rot"][0, 30:] == -1).all()
    mono = {k: v for k, v in fp[0].items() if k != "kp_ur"}            # kp_ur NULL
    g0 = check(ctx, fs, [mono])
    g1 = check(ctx, fs, [dict(fp[0], kp_ur=np.full(513, -1.0))])
    assert g0["match"].tobytes() == g1["match"].tobytes() and (g0["n_gated"] == 0).all()
    plain = [{k: v for k, v in fs[0].items() if k != "pt_angle"}]     # no angles: no orientation check, kp_angle not needed
    g2 = check(ctx, plain, [{k: v for k, v in fp[0].items() if k != "kp_angle"}])
    assert g2["counts"][0, 3] == 0
    check(ctx, [fs[0], ls[0]], [fp[0], dict(lp[0], set=1)], baseline=0.25, ratio=0.6, r_near=1.5, r_wide=6.0, cos_near=0.9, th_dist=60)
    check(ctx, [fs[0], ls[0]], [dict(fp[0], th=15.0), dict(lp[0], set=1, th=0.5)], th_dist=0)
    check(ctx, [fs[0], ls[0]], [dict(fp[0], th=2.0), dict(lp[0], set=1, th=5.0)], th_dist=256, ratio=1e300)


def test_capacity_and_validation_through_a_live_context(ctx, hip_lib):
    E = hip_lib.YgzHipError
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    fs, fp = st.frame_scene(20, 30, 81)
    ls, lp = st.local_scene(20, 30, 82)
    s, p, sl, pl = fs[0], fp[0], ls[0], lp[0]
    call = ctx.stereo_track_search

    def rc(fn):
        with pytest.raises(E) as e:
            fn()
        return e.value.code
    assert rc(lambda: call([s], [p] * (hip_lib.STRACK_MAX_PROBLEMS + 1), K4)) == CAP
    assert rc(lambda: call([s] * (hip_lib.STRACK_MAX_SETS + 1), [p], K4)) == CAP
    n = hip_lib.STRACK_MAX_PAIRS // 2 + 1
    big = dict(pw=np.ones((n, 3)), pt_desc=np.zeros((n, 32), np.uint8), pt_level=np.zeros(n, np.int32))
    q = {k: v for k, v in p.items() if k not in ("pt_skip", "kp_angle")}
    assert rc(lambda: call([big], [q, q], K4)) == CAP
    m = ctx.cells + 1
    wide = dict(T=p["T"], th=7.0, kp_px=np.zeros((m, 2)), kp_level=np.zeros(m, np.int32), kp_desc=np.zeros((m, 32), np.uint8), kp_angle=np.zeros(m))
    assert rc(lambda: call([s], [wide], K4)) == CAP
    assert rc(lambda: call([s], [], K4)) == INV and rc(lambda: call([], [p], K4)) == INV
    assert rc(lambda: call([s], [dict(p, set=1)], K4)) == INV and rc(lambda: call([s], [dict(p, set=-1)], K4)) == INV
    assert rc(lambda: call([s], [dict(p, mode=2)], K4)) == INV and rc(lambda: call([s], [dict(p, direction=2)], K4)) == INV
    assert rc(lambda: call([s], [dict(p, th=0.0)], K4)) == INV and rc(lambda: call([s], [dict(p, th=float("nan"))], K4)) == INV
    assert rc(lambda: call([s], [dict(p, mode=1)], K4)) == INV                                             # a FRAME set read by a LOCAL problem
    assert rc(lambda: call([sl], [dict(pl, mode=0)], K4)) == INV
    assert rc(lambda: call([s], [{k: v for k, v in p.items() if k != "kp_angle"}], K4)) == INV
    assert rc(lambda: call([s], [dict(p, kp_level=np.full(30, 3))], K4)) == INV                            # outside the 3-level pyramid
    assert rc(lambda: call([dict(s, pt_level=np.full(20, 3))], [p], K4)) == INV
    assert rc(lambda: call([dict(s, pt_level=np.full(20, -1))], [p], K4)) == INV
    assert rc(lambda: call([s], [dict(p, kp_ur=np.full(30, np.nan))], K4)) == INV
    assert rc(lambda: call([s], [dict(p, kp_angle=np.full(30, np.inf))], K4)) == INV
    assert rc(lambda: call([dict(s, pt_angle=np.full(20, np.nan))], [p], K4)) == INV
    assert rc(lambda: call([s], [dict(p, T=[0, 0, 0, np.inf, 0, 0, 0])], K4)) == INV
    assert rc(lambda: call([dict(s, pw=np.full((20, 3), np.nan))], [p], K4)) == INV
    assert rc(lambda: call([dict(sl, pt_dmax=np.full(20, np.inf))], [pl], K4)) == INV
    assert rc(lambda: call([dict(sl, pt_normal=np.full((20, 3), np.nan))], [pl], K4)) == INV
    assert rc(lambda: call([s], [p], (0.0, 1.0, 1.0, 1.0))) == INV
    for bad in (dict(th_dist=-1), dict(th_dist=257), dict(baseline=0.0), dict(ratio=0.0), dict(r_near=0.0), dict(r_wide=-1.0),
                dict(ratio=float("nan"))):
        assert rc(lambda: call([s], [p], K4, **bad)) == INV, bad
    check(ctx, [s, sl], [p, dict(pl, set=1)])                          # the context still works after the refusals
