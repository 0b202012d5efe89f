"""Stereo reference-keyframe tracking on resident slots on the MI355X (ygz_slam_amd/csrc/srk.hip: k_srk_gather, k_srk_resolve, k_srk_scatter
around k_bow_transform, k_bow_match<0> and k_pose_opt) against the composition tests/srk_ref.py: EVERY output of EVERY frame is bit-identical
to the composition run on the arrays fetched from the same slots (get_keypoints_batch, get_keypoint_depths), doubles compared as their 64
bits.

One QVGA context with 3 levels and 12 slots (768 cells) and one with a single level, each with a synthetic vocabulary loaded.  The pictures are
windows of one texture that move by 3 pixels per frame; the keypoints are hand-placed lattice points that move with it
(describe_given_angle), 60 % of them with the constant depth of the scene (set_keypoint_depths).  A keyframe's point set is made of its slot's
keypoints un-projected at the scene's depth, in a shuffled order, so that a set index is not a keypoint index.  No case is left out of the
comparison."""
import numpy as np
import pytest

import bow_cases as bc
import fixtures
import popt_ref
import slm_ref as sl
import srk_ref as sk
import stereo_ref as sr
from conftest import make_ctx

pytestmark = pytest.mark.gpu

W, H, SHIFT, Z = 320, 240, 3, 4.0
K = popt_ref.DEFAULT_K
SIZES = (1, 63, 64, 65, 255, 256, 257, 768)
DOUBLES = ("T_out", "chi2", "cost_initial", "cost_final", "lambda")
INTS = ("status", "counts", "kp_point", "prior", "outlier", "inliers", "rounds_run", "round_status", "lm_iterations", "match12", "outcome", "rot")
FREE = 11                                                              # a slot no test ever uploads to


def same(got, want):
    for k in DOUBLES + INTS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if k in DOUBLES:
            g, w = g.view(np.uint64), w.view(np.uint64)
        else:
            assert g.dtype == w.dtype, (k, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:6]
            raise AssertionError((k, bad.tolist(), [got[k][tuple(b)] for b in bad], [want[k][tuple(b)] for b in bad]))


def frame_slice(o, f):
    return {k: v[f:f + 1] for k, v in o.items()}


def shifted(pixels, dy=0.0):
    """the world -> camera pose that moves the projections of the scene's depth by `pixels` along x (and dy along y)"""
    return np.array([0, 0, 0, 1.0, pixels * Z / K[0], dy * Z / K[1], 0])


def point_set(fr, seed, world_shift=0.0):
    """(set, kf_point): one point on every keypoint of a slot whose picture is `world_shift` pixels into the sequence, in a shuffled order:
    kf_point[i] is the set index of keypoint i's point.  The set has every field ygz_hip_stereo_local_map_slots reads too"""
    n = len(fr["level"])
    order = np.random.default_rng(seed).permutation(n).astype(np.int32)    # set index -> keypoint
    px = fr["px"][order] + [world_shift, 0.0]
    Pc = np.stack([(px[:, 0] - K[2]) / K[0] * Z, (px[:, 1] - K[3]) / K[1] * Z, np.full(n, Z)], 1)
    d = np.linalg.norm(Pc, axis=1)
    kf_point = np.empty(n, np.int32)
    kf_point[order] = np.arange(n, dtype=np.int32)
    s = dict(pw=Pc, pt_desc=fr["desc"][order].copy(), pt_dmax=2.0 ** fr["level"][order] * 0.9 * d, pt_normal=Pc / d[:, None])
    return s, kf_point


class Rig(object):
    """a context with a vocabulary, the frames in its slots as the composition wants them, and the call on both sides"""

    def __init__(self, hip_lib, levels, blob):
        self.ctx = make_ctx(hip_lib, width=W, height=H, levels=levels, max_frames=12)
        self.levels, self.frames = levels, {}
        self.vo = sk.oracle().vocab_parse(blob)
        assert self.ctx.vocab_load(blob) == (self.vo.k, self.vo.L, self.vo.n_nodes, self.vo.n_words)
        self.src = sr.texture(W + SHIFT * 8, H, 5)
        px, level = sr.lattice(W + SHIFT * 8, H, 9)
        ok = (px[:, 1] >= 12) & (px[:, 1] <= H - 12)
        px, level = px[ok], level[ok]
        order = np.random.default_rng(9).permutation(len(level))
        self.lat_px, self.lat_level = px[order], (level[order] % levels).astype(np.int32)
        self.lat_angle = (np.random.default_rng(10).integers(0, 1440, len(level)) / 4.0).astype(np.float32)
        self.ready = False

    def put(self, slot, k, n=None, depth=None, has_mp=None, px=None, level=None, angle=None, seed=0):
        """frame k of the sequence into `slot` with its first n lattice keypoints (the first 700 of those inside the picture when n is None)"""
        rng = np.random.default_rng(1000 + 17 * slot + seed)
        self.ctx.upload_gray(slot, np.ascontiguousarray(self.src[:, k * SHIFT:k * SHIFT + W]))
        self.ctx.build_pyramid(slot, 1)
        if px is None:
            x = self.lat_px[:, 0] - k * SHIFT
            keep = np.flatnonzero((x >= 12) & (x <= W - 12))[:n if n is not None else 700]
            px, level = np.stack([x[keep], self.lat_px[keep, 1]], 1), self.lat_level[keep]
            angle = self.lat_angle[keep] if angle is None else angle
        m = len(level)
        assert n is None or m == n
        depth = np.full(m, Z) if depth is None else depth
        has_mp = (rng.uniform(size=m) < 0.6).astype(np.uint8) if has_mp is None else has_mp
        self.ctx.describe_given_angle(slot, px, level, np.asarray(angle, np.float32))
        self.ctx.set_keypoint_depths(slot, np.asarray(depth, np.float64), np.asarray(has_mp, np.uint8))
        kp = self.ctx.get_keypoints_batch(slot, 1)
        cnt = int(kp["count"][0])
        d, hm = self.ctx.get_keypoint_depths(slot)
        assert cnt == m and len(d) == m
        self.frames[slot] = dict(px=kp["px"][0, :cnt].copy(), level=kp["level"][0, :cnt].copy(), angle=kp["angle"][0, :cnt].copy(),
                                 desc=kp["desc"][0, :cnt].copy(), depth=d, has_mp=hm)
        return self.frames[slot]

    def sequence(self):
        if not self.ready:
            for k in range(6):
                self.put(k, k)
            self.ready = True

    def rows(self, kf_points):
        """[n_kf, cells] from a list of arrays by keyframe keypoint"""
        out = np.full((len(kf_points), self.ctx.cells), -1, np.int32)
        for k, p in enumerate(kf_points):
            out[k, :len(p)] = p
        return out

    def both(self, sets, kf_slot, kf_set, kf_points, slots, kf, T, pose=None, **kw):
        fields = dict(kw)
        if pose:
            fields.update({"pose_" + k: v for k, v in pose.items()})
        rows = self.rows(kf_points)
        got = self.ctx.stereo_ref_keyframe_slots(sets, kf_slot, kf_set, rows, slots, kf, T, **fields)
        want = sk.ref_keyframe(self.frames, sets, kf_slot, kf_set, rows, slots, kf, T, self.vo, self.ctx.cells, K=K,
                               pose=None if pose is None else sk.pose_params(kw.get("baseline", 0.1), **pose), **kw)
        same(got, want)
        return got


@pytest.fixture(scope="module")
def rig(hip_lib):
    r = Rig(hip_lib, 3, bc.ragged_vocabulary())
    yield r
    r.ctx.close()


@pytest.fixture(scope="module")
def rig1(hip_lib):
    r = Rig(hip_lib, 1, fixtures.synthetic_vocabulary(k=3, L=6, seed=9))
    yield r
    r.ctx.close()


def test_frames_on_one_keyframe_a_second_call_and_other_bow_states(rig):
    """the first call of the module comes without any ygz_hip_compute_bow; a compute_bow with another levelsup in between changes nothing"""
    rig.sequence()
    assert rig.ctx.cells == 768
    s, kfp = point_set(rig.frames[0], 1)
    one = rig.both([s], [0], [0], [kfp], [1], [0], [shifted(-SHIFT + 0.4)], levelsup=1)
    assert one["status"][0] == 0 and one["counts"][0, 7] > 100 and one["inliers"][0] > 60              # the case is about something
    slots = [1, 2, 3, 0]                                                                               # the keyframe against itself too
    T = np.stack([shifted(-SHIFT + 0.4), shifted(-2 * SHIFT, 0.3), shifted(-3 * SHIFT - 0.5), shifted(0.2)])
    got = rig.both([s], [0], [0], [kfp], slots, [0] * 4, T, levelsup=1)
    assert (got["status"] == 0).all() and got["counts"][:, 7].min() > 100
    same(frame_slice(got, 0), one)
    three = rig.both([s], [0], [0], [kfp], slots[:3], [0] * 3, T[:3], levelsup=1)
    same(three, {k: v[:3] for k, v in got.items()})
    again = rig.ctx.stereo_ref_keyframe_slots([s], [0], [0], rig.rows([kfp]), slots, [0] * 4, T, levelsup=1)
    same(again, got)
    rig.ctx.compute_bow(0, 6, 3)
    same(rig.ctx.stereo_ref_keyframe_slots([s], [0], [0], rig.rows([kfp]), slots, [0] * 4, T, levelsup=1), got)
    assert np.abs(got["T_out"][:3, 4] + np.arange(1, 4) * SHIFT * Z / K[0]).max() < 2e-3              # the pictures move by SHIFT pixels
    # the call leaves the BoW of its slots where ygz_hip_compute_bow leaves it
    node = rig.ctx.get_bow(2)[2]
    assert np.array_equal(node, sk.nodes(rig.vo, rig.frames[2]["desc"], 1))


def kf_variants(rig, slot, seed, world_shift):
    """(set, the kf_point rows all -1, partial, full, with duplicate points) of a slot"""
    s, full = point_set(rig.frames[slot], seed, world_shift)
    n = len(full)
    partial = full.copy()
    partial[1::3] = -1
    dup = full.copy()
    dup[:60] = np.repeat(full[:60:2], 2)                                 # keypoints 2 i and 2 i + 1 carry the same point
    return s, [np.full(n, -1, np.int32), partial, full, dup]


def test_65_frames_four_kf_point_forms_and_a_slot_with_two_poses(rig):
    rig.sequence()
    rng = np.random.default_rng(21)
    s0, v0 = kf_variants(rig, 0, 2, 0.0)
    s4, v4 = kf_variants(rig, 4, 3, 4.0 * SHIFT)
    kf_slot, kf_set, kf_points = [0] * 4 + [4] * 4, [0] * 4 + [1] * 4, v0 + v4
    slots = [int(rng.integers(0, 6)) for _ in range(65)]
    slots[:2] = [3, 3]                                                   # the same slot twice with two poses
    kf = [int(rng.integers(0, 8)) for _ in range(65)]
    kf[:2] = [2, 2]
    T = np.stack([shifted(-s_ * SHIFT + rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)) for s_ in slots])
    got = rig.both([s0, s4], kf_slot, kf_set, kf_points, slots, kf, T, levelsup=1)
    none = np.isin(kf, (0, 4))
    assert (got["status"][none] == 1).all() and (got["T_out"][none] == T[none]).all() and (got["counts"][none, 1] == 0).all()
    assert (got["status"] == 0).sum() > 30 and len(set(zip(slots, kf))) > 25
    assert got["T_out"][0].tobytes() != got["T_out"][1].tobytes()
    d = np.flatnonzero(np.isin(kf, (3, 7)))[0]                            # duplicate points: both keypoints may hold the point
    pts = got["kp_point"][d][got["kp_point"][d] >= 0]
    assert len(pts) > len(np.unique(pts))


@pytest.mark.parametrize("k", range(len(SIZES)))
def test_wavefront_and_tile_edges(rig, k):
    rig.sequence()
    n1, n2 = SIZES[k], SIZES[(k + 3) % len(SIZES)]
    rig.put(6, 0, n=n1)
    rig.put(7, 1, n=n2)
    s6, p6 = point_set(rig.frames[6], 10 + k)
    s0, p0 = point_set(rig.frames[0], 5)
    T = np.stack([shifted(-SHIFT), shifted(-SHIFT + 0.3), shifted(0.2), shifted(0.0)])
    got = rig.both([s6, s0], [6, 0], [0, 1], [p6, p0], [7, 7, 6, 1], [0, 1, 1, 0], T, levelsup=4, min_matches=1, pose=dict(min_edges=1))
    assert got["counts"][:, 0].tolist() == [n1, len(p0), len(p0), n1] and got["counts"][:, 2].tolist() == [n2, n2, n1, len(rig.frames[1]["level"])]
    assert got["counts"][:, 4].sum() > 1


@pytest.mark.parametrize("n", (64, 257))
def test_single_level_pyramid(rig1, n):
    rig1.put(0, 0)
    rig1.put(1, 1)
    rig1.put(2, 0, n=n)
    s, kfp = point_set(rig1.frames[0], 6)
    got = rig1.both([s], [0], [0], [kfp], [0, 1, 2], [0, 0, 0], np.stack([shifted(0.2), shifted(-SHIFT), shifted(0.0)]))
    assert got["counts"][0, 7] > 100 and len(np.unique(sk.nodes(rig1.vo, rig1.frames[0]["desc"], 4))) > 1


def test_contention_two_features_on_one_keypoint(rig):
    """every second lattice keypoint of the keyframe stands twice, at the same pixel, level and angle: both copies find the same frame
    keypoint, the first keeps it and the second loses the claim"""
    rig.sequence()
    f0 = rig.frames[0]
    n = 300
    twice = np.concatenate([np.arange(n), np.arange(0, n, 2)])
    fr = rig.put(8, 0, px=f0["px"][twice], level=f0["level"][twice], angle=f0["angle"][twice], has_mp=np.ones(len(twice), np.uint8))
    s, kfp = point_set(fr, 31)
    got = rig.both([s], [8], [0], [kfp], [0, 1], [0, 0], np.stack([shifted(0.2), shifted(-SHIFT)]), levelsup=1)
    oc = got["outcome"][0, :len(twice)]
    lost = np.flatnonzero(oc == sk.LOST_CLAIM)
    assert len(lost) > 60 and (lost >= n).all() and got["counts"][0, 5] == len(lost) and (got["match12"][0, lost] == -1).all()
    first = twice[lost]                                                  # the copy that kept the keypoint
    assert (oc[first] != sk.LOST_CLAIM).all()
    assert got["counts"][1, 5] > 30


def test_orientation_removes_matches(rig):
    """keyframe angles turned by 0, 20 and 100 degrees in the parts 60 / 30 / 10 %, and the descriptors with them (th_low 256, the ratio rule
    off, one node, so every feature matches its nearest): the matches outside the fullest bins are removed; without the check they stay"""
    rig.sequence()
    f0 = rig.frames[0]
    n = len(f0["level"])
    rng = np.random.default_rng(41)
    turn = rng.choice([0.0, 20.0, 100.0], n, p=[0.6, 0.3, 0.1])
    fr = rig.put(9, 0, px=f0["px"], level=f0["level"], angle=((f0["angle"].astype(np.float64) + turn) % 360.0).astype(np.float32))
    s, kfp = point_set(fr, 32)
    T = np.stack([shifted(0.2), shifted(-SHIFT)])
    got = rig.both([s], [9], [0], [kfp], [0, 1], [0, 0], T, levelsup=4, th_low=256, knn_ratio=1.0)
    assert got["counts"][0, 6] > 5 and (got["outcome"][0] == sk.ORIENTATION).sum() == got["counts"][0, 6] and got["rot"][0, 30] == 0
    off = rig.both([s], [9], [0], [kfp], [0, 1], [0, 0], T, levelsup=4, th_low=256, knn_ratio=1.0, check_orientation=0)
    assert (off["counts"][:, 6] == 0).all() and (off["rot"][:, :30] == 0).all() and (off["rot"][:, 30:] == -1).all()
    assert off["counts"][0, 7] == got["counts"][0, 7] + got["counts"][0, 6]


def test_mono_keypoints(rig):
    """a keypoint whose u - bf / depth is negative counts as mono; a flag of 0 with a depth, and a NaN depth, have no depth"""
    rig.sequence()
    n = len(rig.frames[1]["level"])
    dc, hc = np.full(n, Z), np.ones(n, np.uint8)
    dc[::4] = 0.05                                                       # bf / 0.05 = 1042 pixels: the right column is far below zero
    dc[1::7] = np.nan
    hc[2::7] = 0
    fr = rig.put(10, 1, depth=dc, has_mp=hc)
    s, kfp = point_set(rig.frames[0], 12)
    got = rig.both([s], [0], [0], [kfp], [10], [0], [shifted(-SHIFT + 0.3)], levelsup=1)
    ur = sk.right_columns(fr["px"], fr["depth"], sk.has_depth(fr["depth"], fr["has_mp"]), 0.1, K)
    near = (fr["depth"] == 0.05) & (fr["has_mp"] != 0)
    assert near.sum() > 50 and (ur[near] < -100).all() and got["counts"][0, 3] == (ur >= 0).sum() < n - near.sum()
    mono = np.flatnonzero((ur < 0) & (got["kp_point"][0, :n] >= 0))
    assert len(mono) > 30 and got["counts"][0, 7] > 100                  # they are matched and went into the optimiser as mono edges


@pytest.mark.parametrize("fields,pose", [(dict(levelsup=0), None), (dict(levelsup=1), None), (dict(levelsup=4), None), (dict(th_low=30), None),
                                         (dict(knn_ratio=1.0), None), (dict(min_matches=0), None), (dict(min_matches=1000), None),
                                         (dict(min_inliers=1000), None), (dict(), dict(rounds=1)),
                                         (dict(baseline=0.3), dict(min_rel_decrease=1e-6, robust_rounds=1))])
def test_other_parameters(rig, fields, pose):
    rig.sequence()
    s, kfp = point_set(rig.frames[0], 13)
    s5, v5 = kf_variants(rig, 5, 14, 5.0 * SHIFT)
    T = np.stack([shifted(-SHIFT + 1.0), shifted(-2 * SHIFT + 0.5), shifted(-5 * SHIFT)])
    f = dict(dict(levelsup=2), **fields)
    got = rig.both([s, s5], [0, 5], [0, 1], [kfp, v5[0]], [1, 2, 5], [0, 0, 1], T, pose=pose, **f)
    if fields.get("min_matches") == 1000:
        assert (got["status"] == 1).all() and (got["T_out"] == T).all() and got["counts"][0, 7] > 100 and not got["outlier"].any()
    elif fields.get("min_matches") == 0:
        assert (got["status"][:2] == 0).all() and got["status"][2] == 2 and got["counts"][2, 7] == 0 and (got["T_out"][2] == T[2]).all()
    elif fields.get("min_inliers") == 1000:
        assert got["status"].tolist() == [2, 2, 1] and (got["T_out"][:2] != T[:2]).any() and got["inliers"][0] > 60
    else:
        assert got["status"].tolist() == [0, 0, 1]
    if pose and pose.get("rounds") == 1:
        assert (got["rounds_run"][:2] == 1).all()


def test_the_prior_feeds_the_local_map_call(rig):
    """the chain: prior goes, with the same set objects, into ygz_hip_stereo_local_map_slots, whose outputs equal slm_ref on that prior"""
    rig.sequence()
    s, kfp = point_set(rig.frames[0], 15)
    slots = [1, 2]
    T = np.stack([shifted(-SHIFT + 0.4), shifted(-2 * SHIFT, 0.3)])
    got = rig.both([s], [0], [0], [kfp], slots, [0, 0], T, levelsup=1)
    prior = got["prior"]
    assert (prior >= 0).sum(1).min() > 60 and ((got["kp_point"] >= 0) & (prior < 0)).sum() == got["outlier"].sum()
    lm = rig.ctx.stereo_local_map_slots([s], slots, [0, 0], got["T_out"], prior)
    frames = {sl_: {k: v for k, v in rig.frames[sl_].items() if k != "angle"} for sl_ in slots}
    want = sl.local_map(frames, [s], slots, [0, 0], got["T_out"], [prior[f, :len(frames[sl_]["level"])] for f, sl_ in enumerate(slots)],
                        cells=rig.ctx.cells, K=K, w=W, h=H, L=rig.levels)
    for k in ("T_out", "chi2", "proj"):
        assert np.array_equal(np.ascontiguousarray(lm[k]).view(np.uint64), np.ascontiguousarray(want[k]).view(np.uint64)), k
    for k in ("status", "counts", "kp_point", "outlier", "inliers", "rounds_run", "match", "reason", "outcome"):
        assert np.array_equal(lm[k], want[k]), k
    assert (lm["counts"][:, 2] == (prior >= 0).sum(1)).all() and (lm["status"] == 0).all()


def test_errors_through_a_live_context(rig, hip_lib):
    rig.sequence()
    E, ctx = hip_lib.YgzHipError, rig.ctx
    s, kfp = point_set(rig.frames[0], 16)
    row = rig.rows([kfp])
    I = sk.IDENTITY

    def code(*a, **kw):
        with pytest.raises(E) as e:
            ctx.stereo_ref_keyframe_slots(*a, **kw)
        return e.value.code
    n = hip_lib.SRK_MAX_FRAMES + 1
    assert code([s], [0], [0], row, [1] * n, [0] * n, np.tile(I, (n, 1)), outputs=False) == hip_lib.E_CAPACITY
    ok = ctx.stereo_ref_keyframe_slots([s], [0], [0], row, [1] * (n - 1), [0] * (n - 1), np.tile(I, (n - 1, 1)), outputs=False)
    assert (ok["status"] == ok["status"][0]).all() and (ok["T_out"] == ok["T_out"][0]).all() and (ok["prior"] == ok["prior"][0]).all()
    m = hip_lib.SRK_MAX_KEYFRAMES + 1
    assert code([s], [0] * m, [0] * m, np.tile(row, (m, 1)), [1], [0], [I], outputs=False) == hip_lib.E_CAPACITY
    at = ctx.stereo_ref_keyframe_slots([s], [0] * (m - 1), [0] * (m - 1), np.tile(row, (m - 1, 1)), [1], [m - 2], [I], outputs=False)
    assert at["status"][0] == ok["status"][0] and (at["T_out"][0] == ok["T_out"][0]).all()
    m = hip_lib.SRK_MAX_SETS + 1
    assert code([s] * m, [0], [0], row, [1], [0], [I], outputs=False) == hip_lib.E_CAPACITY
    at = ctx.stereo_ref_keyframe_slots([s] * (m - 1), [0], [m - 2], row, [1], [0], [I], outputs=False)
    assert at["status"][0] == ok["status"][0] and (at["T_out"][0] == ok["T_out"][0]).all()
    assert code([s], [0], [0], row, [12], [0], [I]) == hip_lib.E_INVALID and code([s], [0], [0], row, [-1], [0], [I]) == hip_lib.E_INVALID
    assert code([s], [12], [0], row, [1], [0], [I]) == hip_lib.E_INVALID and code([s], [-1], [0], row, [1], [0], [I]) == hip_lib.E_INVALID
    assert code([s], [0], [1], row, [1], [0], [I]) == hip_lib.E_INVALID and code([s], [0], [-1], row, [1], [0], [I]) == hip_lib.E_INVALID
    assert code([s], [0], [0], row, [1], [1], [I]) == hip_lib.E_INVALID and code([s], [0], [0], row, [1], [-1], [I]) == hip_lib.E_INVALID
    assert code([s], [0], [0], row, [], [], np.zeros((0, 7))) == hip_lib.E_INVALID
    assert code([], [0], [0], row, [1], [0], [I]) == hip_lib.E_INVALID
    assert code([s], [], [], np.zeros((0, ctx.cells), np.int32), [1], [0], [I]) == hip_lib.E_INVALID
    bad = I.copy()
    bad[5] = np.inf
    assert code([s], [0], [0], row, [1], [0], [bad]) == hip_lib.E_INVALID
    nan = dict(s, pw=s["pw"].copy())
    nan["pw"][3, 1] = np.nan
    assert code([nan], [0], [0], row, [1], [0], [I]) == hip_lib.E_INVALID
    for v, at_ in ((len(kfp), 0), (-2, 5), (0, ctx.cells - 1)):
        r = row.copy()
        r[0, at_] = v
        if v == 0:
            ctx.stereo_ref_keyframe_slots([s], [0], [0], r, [1], [0], [I])     # in range: accepted, also past the last keypoint
        else:
            assert code([s], [0], [0], r, [1], [0], [I]) == hip_lib.E_INVALID, v
    assert code([dict()], [0], [0], np.zeros((1, ctx.cells), np.int32), [1], [0], [I]) == hip_lib.E_INVALID     # no point to name
    empty = ctx.stereo_ref_keyframe_slots([dict()], [0], [0], np.full((1, ctx.cells), -1, np.int32), [1], [0], [I])
    assert empty["status"][0] == 1 and (empty["T_out"][0] == I).all()
    for f in (dict(baseline=0.0), dict(baseline=np.nan), dict(th_low=257), dict(th_low=-1), dict(knn_ratio=0.0), dict(knn_ratio=np.inf),
              dict(levelsup=-1), dict(min_matches=-1), dict(min_inliers=-1), dict(pose_rounds=0), dict(pose_rounds=9), dict(pose_iterations=65),
              dict(pose_max_trials=0), dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=np.inf)):
        assert code([s], [0], [0], row, [1], [0], [I], **f) == hip_lib.E_INVALID, f
    assert code([s], [0], [0], row, [FREE], [0], [I]) == hip_lib.E_STATE and code([s], [FREE], [0], row, [1], [0], [I]) == hip_lib.E_STATE
    rig.both([s], [0], [0], [kfp], [1], [0], [shifted(-SHIFT + 0.2)], levelsup=1)      # the context is none the worse for it


def test_state_errors_without_vocabulary_and_without_depths(hip_lib):
    ctx = make_ctx(hip_lib, width=W, height=H, levels=3, max_frames=2)
    try:
        ctx.upload_gray(0, sr.texture(W, H, 5))
        ctx.build_pyramid(0, 1)
        s = dict(pw=np.array([[0.0, 0, 4]]))
        row = np.full((1, ctx.cells), -1, np.int32)
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.stereo_ref_keyframe_slots([s], [0], [0], row, [0], [0], [sk.IDENTITY])
        assert e.value.code == hip_lib.E_STATE                             # no vocabulary
        ctx.vocab_load(bc.ragged_vocabulary())
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.stereo_ref_keyframe_slots([s], [0], [0], row, [0], [0], [sk.IDENTITY])
        assert e.value.code == hip_lib.E_STATE                             # depths never written
    finally:
        ctx.close()
