"""Stereo relocalisation on resident slots on the MI355X (ygz_slam_amd/csrc/srl.hip: k_srl_gather, k_srl_resolve, k_srl_sets, k_srl_edges,
k_srl_scatter, k_srl_pick around k_bow_transform, k_bow_match<0>, k_pnp_solve, k_pnp_score, k_pnp_select and k_pose_opt) against the
composition tests/srl_ref.py: EVERY output of EVERY problem is bit-identical to the composition run on the arrays fetched from the same slots,
doubles compared as their 64 bits.

The rig is that of tests/test_gpu_srk.py: one QVGA context with 3 levels and 12 slots (768 cells) and a synthetic vocabulary; the pictures are
windows of one texture that move by 3 pixels per frame, the keypoints hand-placed lattice points that move with it, a keyframe's point set its
keypoints un-projected at the scene's depth in a shuffled order.  A lost frame has no entry pose; the truth of frame k against the points of
keyframe 0 is a shift by -3 k pixels.  Where a case needs an exact number of associations, the keyframe's kf_point row is cut to that many of
the features the composition itself associates (a feature's match does not depend on the other features), and the count is asserted."""
import ctypes as C

import numpy as np
import pytest

import bow_cases as bc
import pnp_ref
import slm_ref as sl
import srk_ref as sk
import srl_ref as rl
import stereo_ref as sr
from conftest import make_ctx
from test_gpu_srk import FREE, H, K, SHIFT, W, Z, Rig, point_set, shifted

pytestmark = pytest.mark.gpu

DOUBLES = ("T_out", "T_pnp", "T_opt", "pnp_R", "pnp_t", "pnp_T_cw", "chi2", "cost_initial", "cost_final", "lambda")
INTS = ("best", "status", "counts", "pnp_success", "pnp_n_inliers", "pnp_best_sample", "pnp_best_solution", "pnp_n_hypotheses", "kp_point",
        "pnp_inlier", "prior", "outlier", "inliers", "rounds_run", "round_status", "lm_iterations", "match12", "outcome", "rot", "sets")
WIDE = dict(levelsup=4, th_low=256, knn_ratio=1.0)                       # every keyframe feature takes its nearest: many associations
NARROW = dict(levelsup=1, min_final_inliers=30)                          # the default gates, with which an unrelated picture matches nothing


def same(got, want, keys=DOUBLES + INTS):
    for k in keys:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if k in DOUBLES:
            g, w = g.view(np.uint64), w.view(np.uint64)
        else:
            assert g.dtype == w.dtype, (k, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:6]
            raise AssertionError((k, bad.tolist(), [got[k][tuple(b)] for b in bad], [want[k][tuple(b)] for b in bad]))


def both(rig, sets, kf_slot, kf_set, kf_points, slots, candidates, pose=None, pnp=None, **kw):
    fields = dict(kw)
    fields.update({"pose_" + k: v for k, v in (pose or {}).items()})
    fields.update({"pnp_" + k: v for k, v in (pnp or {}).items()})
    rows = rig.rows(kf_points)
    got = rig.ctx.stereo_relocalize_slots(sets, kf_slot, kf_set, rows, slots, candidates, **fields)
    want = rl.relocalize(rig.frames, sets, kf_slot, kf_set, rows, slots, candidates, rig.vo, rig.ctx.cells, K=K, pnp=pnp,
                         pose=None if pose is None else sk.pose_params(kw.get("baseline", 0.1), **pose), **kw)
    same(got, want)
    return got


def problem_slice(o, q):
    return {k: v[q:q + 1] for k, v in o.items() if k not in ("T_out", "best", "cand_off")}


def associated(rig, kf_slot, slot, kfp, s, **kw):
    """the keyframe features the composition associates with a keypoint of the frame, ascending"""
    a = rl.associate(rig.frames[kf_slot], rig.frames[slot], kfp, s, rig.vo, K, dict(rl.DEFAULTS, **kw))
    return np.flatnonzero(a["match12"] >= 0)


def cut(kfp, feats):
    """kf_point with a point on the given features only"""
    out = np.full(len(kfp), -1, np.int32)
    out[feats] = kfp[feats]
    return out


def other_picture(rig, slot, seed):
    """a slot with the lattice keypoints on an unrelated texture: its descriptors match nothing of the sequence"""
    keep, rig.src = rig.src, sr.texture(W + SHIFT * 8, H, seed)
    try:
        return rig.put(slot, 0)
    finally:
        rig.src = keep


def displaced(s, seed, part=1.0):
    """the set with `part` of its points moved by up to a metre each, every one on its own"""
    rng = np.random.default_rng(seed)
    pw = s["pw"].copy()
    move = rng.uniform(size=len(pw)) < part
    pw[move] += rng.uniform(-1.0, 1.0, (int(move.sum()), 3))
    return dict(s, pw=pw)


@pytest.fixture(scope="module")
def rig(hip_lib):
    r = Rig(hip_lib, 3, bc.ragged_vocabulary())
    yield r
    r.ctx.close()


def test_every_status_the_winner_and_a_second_call(rig):
    """3 frames x 3 candidates among five keyframes: the true one, the same once more, an unrelated picture, the true slot with a displaced
    set, the true slot with 25 associations (fewer than min_final_inliers).  Frames 0 and 2 share slot 1; four keyframes share slot 0"""
    rig.sequence()
    assert rig.ctx.cells == 768
    other_picture(rig, 6, 77)
    s0, p0 = point_set(rig.frames[0], 1)
    s6, p6 = point_set(rig.frames[6], 2)
    feats = associated(rig, 0, 2, p0, s0, **NARROW)
    assert len(feats) >= 60
    few = cut(p0, feats[:25])
    sets, kf_slot, kf_set, kfp = [s0, s6, displaced(s0, 3)], [0, 0, 6, 0, 0], [0, 0, 1, 2, 0], [p0, p0, p6, p0, few]
    TRUE, AGAIN, OTHER, MOVED, FEW = range(5)
    cands = [[OTHER, MOVED, TRUE], [FEW, TRUE, OTHER], [AGAIN, TRUE, MOVED]]
    got = both(rig, sets, kf_slot, kf_set, kfp, [1, 2, 1], cands, **NARROW)
    assert got["status"].tolist() == [1, 2, 0, 3, 0, 1, 0, 0, 2] and set(got["status"]) == {0, 1, 2, 3}
    assert got["best"].tolist() == [2, 4, 6]                             # the first success in the caller's order, not the best one
    assert got["counts"][3, 7] == 25 and got["pnp_success"][3] == 1 and got["inliers"][3] <= 25 and got["counts"][0, 7] < 15
    for f, q in enumerate(got["best"]):
        assert got["T_out"][f].tobytes() == got["T_opt"][q].tobytes()
    assert np.abs(got["T_out"][:, 4] + np.array([1, 2, 1]) * SHIFT * Z / K[0]).max() < 2e-3              # the pictures move by SHIFT pixels
    assert (got["T_pnp"][0] == rl.IDENTITY).all() and (got["T_opt"][0] == rl.IDENTITY).all() and got["pnp_n_hypotheses"][0] == 0
    assert got["T_opt"][1].tobytes() == got["T_pnp"][1].tobytes() and got["inliers"][1] == 0 and not got["outlier"][1].any()
    assert not got["pnp_inlier"][0].any() and (got["prior"][0] == -1).all() and not got["sets"][0].any()
    assert got["T_opt"][6].tobytes() == got["T_opt"][7].tobytes() == got["T_opt"][2].tobytes()      # one problem, wherever it stands
    again = rig.ctx.stereo_relocalize_slots(sets, kf_slot, kf_set, rig.rows(kfp), [1, 2, 1], cands, **NARROW)
    same(again, got)
    # a frame without candidates, and without a winner
    none = both(rig, sets, kf_slot, kf_set, kfp, [1, 2, 3], [[OTHER], [], [MOVED, OTHER]], **NARROW)
    assert none["best"].tolist() == [-1, -1, -1] and (none["T_out"] == rl.IDENTITY).all()
    # NULL for the optional outputs changes nothing of the others
    lean = rig.ctx.stereo_relocalize_slots(sets, kf_slot, kf_set, rig.rows(kfp), [1, 2, 1], cands, outputs=False, **NARROW)
    same(lean, got, ("T_out", "best", "status", "T_opt", "prior"))
    # the default parameters on the plain case
    both(rig, [s0], [0], [0], [p0], [1, 2, 3], [[0], [0], [0]])


@pytest.mark.parametrize("n", (14, 15, 16, 63, 64, 65, 255, 256, 257))
def test_association_counts_at_the_tile_and_wavefront_edges(rig, n):
    rig.sequence()
    s0, p0 = point_set(rig.frames[0], 4)
    feats = associated(rig, 0, 1, p0, s0, **WIDE)
    assert len(feats) >= 257
    got = both(rig, [s0], [0, 0], [0, 0], [cut(p0, feats[:n]), p0], [1, 1], [[0], [1, 0]], min_final_inliers=10, **WIDE)
    assert got["counts"][:, 7].tolist() == [n, len(feats), n]
    assert (got["status"][0] == 1) == (n < 15) and got["pnp_n_inliers"][0] <= n
    same(problem_slice(got, 0), problem_slice(got, 2), [k for k in DOUBLES + INTS if k not in ("T_out", "best")])


@pytest.mark.parametrize("it", (1, 63, 64, 65, 300))
def test_ransac_iteration_edges(rig, it):
    rig.sequence()
    s0, p0 = point_set(rig.frames[0], 5)
    feats = associated(rig, 0, 2, p0, s0, **WIDE)
    got = both(rig, [s0], [0], [0], [cut(p0, feats[:65])], [2], [[0]], pnp=dict(max_iter=it), min_final_inliers=10, **WIDE)
    assert got["counts"][0, 7] == 65 and got["sets"].shape == (1, it, 3)
    assert np.array_equal(got["sets"][0], pnp_ref.sample_sets(65, it)) and len(np.unique(got["sets"][0])) > min(it, 3)


def test_wrong_kf_point_entries(rig):
    """30 % of the keyframe's entries name another point of the set: the PnP leaves them out, the optimiser sees inliers only"""
    rig.sequence()
    s0, p0 = point_set(rig.frames[0], 6)
    rng = np.random.default_rng(7)
    wrong = rng.uniform(size=len(p0)) < 0.3
    bad = p0.copy()
    bad[wrong] = (p0[wrong] + rng.integers(1, len(p0) - 1, int(wrong.sum()))) % len(p0)
    got = both(rig, [s0], [0], [0], [bad], [1, 2], [[0], [0]], **WIDE)
    assert (got["status"] == 0).all()                                   # the reference itself (got equals it) still relocalises
    for q, slot in enumerate((1, 2)):
        kp = got["kp_point"][q]
        named_wrong = np.isin(kp, bad[wrong]) & ~np.isin(kp, bad[~wrong]) & (kp >= 0)
        assert named_wrong.sum() > 30 and not got["pnp_inlier"][q][named_wrong].any()
        inl = got["pnp_inlier"][q] != 0
        assert got["pnp_n_inliers"][q] == inl.sum() and ((got["chi2"][q] >= 0) == inl).all() and not got["outlier"][q][~inl].any()
        assert ((got["prior"][q] == kp) | (got["prior"][q] == -1)).all() and ((got["prior"][q] >= 0) == (inl & (got["outlier"][q] == 0))).all()
        assert got["inliers"][q] == (got["prior"][q] >= 0).sum()


def test_mono_keypoints_orientation_and_claim(rig):
    rig.sequence()
    f0, f1 = rig.frames[0], rig.frames[1]
    n = len(f1["level"])
    rig.put(7, 1, depth=np.where(np.arange(n) % 2, 0.0, -1.0), has_mp=np.ones(n, np.uint8))       # all depths <= 0: every edge is mono
    m = len(f0["level"])
    turn = np.random.default_rng(41).choice([0.0, 20.0, 100.0], m, p=[0.6, 0.3, 0.1])
    turned = rig.put(9, 0, px=f0["px"], level=f0["level"], angle=((f0["angle"].astype(np.float64) + turn) % 360.0).astype(np.float32))
    twice = np.concatenate([np.arange(300), np.arange(0, 300, 2)])
    doubled = rig.put(8, 0, px=f0["px"][twice], level=f0["level"][twice], angle=f0["angle"][twice], has_mp=np.ones(len(twice), np.uint8))
    s0, p0 = point_set(f0, 8)
    s9, p9 = point_set(turned, 9)
    s8, p8 = point_set(doubled, 10)
    got = both(rig, [s0, s9, s8], [0, 9, 8], [0, 1, 2], [p0, p9, p8], [7, 1], [[0, 1, 2], [1, 2]], min_final_inliers=20, **WIDE)
    assert (got["counts"][:3, 3] == 0).all() and got["status"][0] == 0 and got["inliers"][0] >= 20      # frame 0: kind 1 only
    assert (got["counts"][[1, 3], 6] > 5).all() and (got["counts"][[1, 3], 7] == got["counts"][[1, 3], 4] - got["counts"][[1, 3], 5] - got["counts"][[1, 3], 6]).all()
    assert (got["counts"][[2, 4], 5] > 30).all() and ((got["outcome"][2] == sk.LOST_CLAIM).sum() == got["counts"][2, 5])
    off = both(rig, [s9], [9], [0], [p9], [1], [[0]], check_orientation=0, min_final_inliers=20, **WIDE)
    assert off["counts"][0, 6] == 0 and off["counts"][0, 7] == got["counts"][3, 7] + got["counts"][3, 6]      # the check removed them before the PnP


def test_a_status_3_problem_feeds_the_local_map_call(rig):
    rig.sequence()
    s0, p0 = point_set(rig.frames[0], 11)
    feats = associated(rig, 0, 2, p0, s0, **WIDE)
    got = both(rig, [s0], [0], [0], [cut(p0, feats[:45])], [2], [[0]], **WIDE)
    assert got["status"][0] == 3 and got["best"][0] == -1 and 10 <= (got["prior"][0] >= 0).sum() == got["inliers"][0] < 50
    prior, T = got["prior"], got["T_opt"]
    lm = rig.ctx.stereo_local_map_slots([s0], [2], [0], T, prior)
    frames = {2: {k: v for k, v in rig.frames[2].items() if k != "angle"}}
    want = sl.local_map(frames, [s0], [2], [0], T, [prior[0, :len(frames[2]["level"])]], cells=rig.ctx.cells, K=K, w=W, h=H, L=rig.levels)
    for k in ("T_out", "chi2", "proj"):
        assert np.array_equal(np.ascontiguousarray(lm[k]).view(np.uint64), np.ascontiguousarray(want[k]).view(np.uint64)), k
    for k in ("status", "counts", "kp_point", "outlier", "inliers", "rounds_run", "match", "reason", "outcome"):
        assert np.array_equal(lm[k], want[k]), k
    assert lm["counts"][0, 2] == (prior >= 0).sum() and lm["status"][0] == 0 and lm["inliers"][0] >= got["inliers"][0]      # the top-up


def test_errors_through_a_live_context(rig, hip_lib):
    rig.sequence()
    E, ctx = hip_lib.YgzHipError, rig.ctx
    s, kfp = point_set(rig.frames[0], 16)
    row = rig.rows([kfp])

    def code(*a, **kw):
        with pytest.raises(E) as e:
            ctx.stereo_relocalize_slots(*a, **kw)
        return e.value.code
    INV, CAP, STATE = hip_lib.E_INVALID, hip_lib.E_CAPACITY, hip_lib.E_STATE
    # in the order of the header comment
    assert code([s], [0], [0], row, [], []) == INV and code([], [0], [0], row, [1], [[0]]) == INV
    assert code([s], [], [], np.zeros((0, ctx.cells), np.int32), [1], [[0]]) == INV
    m = hip_lib.SRL_MAX_SETS + 1
    assert code([s] * m, [0], [0], row, [1], [[0]], outputs=False) == CAP
    m = hip_lib.SRL_MAX_KEYFRAMES + 1
    assert code([s], [0] * m, [0] * m, np.tile(row, (m, 1)), [1], [[0]], outputs=False) == CAP
    n = hip_lib.SRL_MAX_FRAMES + 1
    assert code([s], [0], [0], row, [1] * n, [[0]] + [[]] * (n - 1), outputs=False) == CAP
    assert code([s], [0], [0], row, [1], [[]]) == INV                                                  # no problem at all
    n = hip_lib.SRL_MAX_PROBLEMS + 1
    assert code([s], [0], [0], row, [1, 1], [[0] * (n - 1), [0]], outputs=False) == CAP
    for f in (dict(baseline=0.0), dict(baseline=np.nan), dict(th_low=257), dict(th_low=-1), dict(knn_ratio=0.0), dict(knn_ratio=np.inf),
              dict(levelsup=-1), dict(min_matches=3), dict(min_final_inliers=-1), dict(pnp_max_iter=0), dict(pnp_max_iter=1025),
              dict(pnp_chi2=0.0), dict(pnp_chi2=np.nan), dict(pnp_min_inliers=-1), dict(pose_rounds=0), dict(pose_rounds=9),
              dict(pose_iterations=65), dict(pose_max_trials=0), dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=np.inf)):
        assert code([s], [0], [0], row, [1], [[0]], **f) == INV, f
    assert code([s], [0], [0], row, [1], [[0] * 76], pnp_max_iter=1024, outputs=False) == CAP            # 76 * 1024 > 76800
    assert code([s], [0], [0], row, [-1], [[0]]) == INV and code([s], [-1], [0], row, [1], [[0]]) == INV
    assert code([s], [0], [1], row, [1], [[0]]) == INV and code([s], [0], [-1], row, [1], [[0]]) == INV
    assert code([s], [0], [0], row, [1], [[1]]) == INV and code([s], [0], [0], row, [1], [[0, -1]]) == INV
    nan = dict(s, pw=s["pw"].copy())
    nan["pw"][3, 1] = np.nan
    assert code([nan], [0], [0], row, [1], [[0]]) == INV
    assert code([s], [0], [0], row, [12], [[0]]) == INV and code([s], [12], [0], row, [1], [[0]]) == INV
    for v, at_ in ((len(kfp), 0), (-2, 5)):
        r = row.copy()
        r[0, at_] = v
        assert code([s], [0], [0], r, [1], [[0]]) == INV, v
    assert code([dict()], [0], [0], np.zeros((1, ctx.cells), np.int32), [1], [[0]]) == INV              # no point to name
    assert code([s], [0], [0], row, [FREE], [[0]]) == STATE and code([s], [FREE], [0], row, [1], [[0]]) == STATE
    # a refused call writes nothing
    hip_lib.srl_argtypes(ctx.lib)
    T_out, best = np.full((1, 7), 5.0), np.full(1, 5, np.int32)
    one, off, ck = np.array([1], np.int32), np.array([0, 1], np.int32), np.array([0], np.int32)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    sa = (hip_lib.StrackPoints * 1)()
    pw = np.ascontiguousarray(s["pw"])
    sa[0].pw, sa[0].n_pt = pw.ctypes.data_as(dp), len(pw)
    p = ctx.default_srl_params(min_matches=3)
    rc = ctx.lib.ygz_hip_stereo_relocalize_slots(ctx._ctx, 1, sa, 1, ck.ctypes.data_as(ip), ck.ctypes.data_as(ip), row.ctypes.data_as(ip), 1,
                                                 one.ctypes.data_as(ip), off.ctypes.data_as(ip), ck.ctypes.data_as(ip), C.byref(p),
                                                 T_out.ctypes.data_as(dp), best.ctypes.data_as(ip), *([None] * 21))
    assert rc == INV and (T_out == 5.0).all() and best[0] == 5
    empty = ctx.stereo_relocalize_slots([dict()], [0], [0], np.full((1, ctx.cells), -1, np.int32), [1], [[0]])
    assert empty["status"][0] == 1 and empty["best"][0] == -1 and (empty["T_out"][0] == rl.IDENTITY).all()
    s0, p0 = point_set(rig.frames[0], 1)
    both(rig, [s0], [0], [0], [p0], [1], [[0]], **WIDE)                  # the context is none the worse for it


def test_state_errors_without_vocabulary_and_without_depths(hip_lib):
    ctx = make_ctx(hip_lib, width=W, height=H, levels=3, max_frames=2)
    try:
        ctx.upload_gray(0, sr.texture(W, H, 5))
        ctx.build_pyramid(0, 1)
        s = dict(pw=np.array([[0.0, 0, 4]]))
        row = np.full((1, ctx.cells), -1, np.int32)
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.stereo_relocalize_slots([s], [0], [0], row, [0], [[0]])
        assert e.value.code == hip_lib.E_STATE                             # no vocabulary
        ctx.vocab_load(bc.ragged_vocabulary())
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.stereo_relocalize_slots([s], [0], [0], row, [0], [[0]])
        assert e.value.code == hip_lib.E_STATE                             # depths never written
    finally:
        ctx.close()
