"""Stereo local-map tracking on resident slots on the MI355X (ygz_slam_amd/csrc/slm.hip: k_slm_gather, k_slm_resolve, k_slm_scatter around
k_strack_search and k_pose_opt) against the composition tests/slm_ref.py: EVERY output of EVERY frame is bit-identical to the composition run
on the arrays fetched from the same slots (get_keypoints_batch, get_keypoint_depths), doubles compared as their 64 bits.

One QVGA context with 3 levels and 10 slots (768 cells) and one with a single level.  The pictures are windows of one texture that move by 3
pixels per frame; the keypoints are hand-placed lattice points that move with it (describe_given_angle), 60 % of them with the constant depth
of the scene (set_keypoint_depths).  A point set is made of a slot's keypoints: un-projected at the scene's depth, the keypoint's descriptor
with some bits flipped, dmax so that the keypoint's level is the predicted one; past the slot's last keypoint the points go round again a
fraction of a pixel off, so that several points want one keypoint.  No case is left out of the comparison."""
import numpy as np
import pytest

import popt_ref
import proj_ref
import slm_ref as sl
import stereo_ref as sr
import strack_ref
from conftest import make_ctx

pytestmark = pytest.mark.gpu

W, H, SHIFT, Z = 320, 240, 3, 4.0
K = popt_ref.DEFAULT_K
PT_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
KP_SIZES = (1, 63, 64, 65, 255, 256, 257)
DOUBLES = ("T_out", "proj", "chi2", "cost_initial", "cost_final", "lambda")
INTS = ("status", "counts", "kp_point", "outlier", "inliers", "rounds_run", "round_status", "lm_iterations", "offsets") + sl.INT_OUTPUTS
FREE = 9                                                               # a slot no test ever uploads to


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
    """frame f of a call's outputs as a call of one frame"""
    a, b = int(o["offsets"][f]), int(o["offsets"][f + 1])
    out = {k: (v[a:b] if k in sl.INT_OUTPUTS + ("proj",) else v[f:f + 1]) for k, v in o.items() if k != "offsets"}
    out["offsets"] = np.array([0, b - a], np.int64)
    return out


def shifted(pixels, dy=0.0):
    """the world -> camera pose that moves the projections of the scene's depth by `pixels` along x (and dy along y)"""
    return np.array([0, 0, 0, 1.0, pixels * Z / K[0], dy * Z / K[1], 0])


def point_set(fr, n_pt, seed, bits=20, start=0):
    """n_pt points on the keypoints start, start + 1, ... of a slot (round again past the last one); (set, the keypoint of every point)"""
    rng = np.random.default_rng(seed)
    n_kp = len(fr["level"])
    j = (start + np.arange(n_pt)) % n_kp
    px = fr["px"][j] + rng.uniform(-0.7, 0.7, (n_pt, 2)) * (np.arange(n_pt) >= n_kp)[:, None]
    Pc = np.stack([(px[:, 0] - K[2]) / K[0] * Z, (px[:, 1] - K[3]) / K[1] * Z, np.full(n_pt, Z)], 1)
    d = np.linalg.norm(Pc, axis=1)
    desc = np.stack([proj_ref.flip_bits(rng, fr["desc"][jj], int(rng.integers(0, bits + 1))) for jj in j])
    return dict(pw=Pc, pt_desc=desc, pt_dmax=2.0 ** fr["level"][j] * 0.9 * d, pt_normal=Pc / d[:, None]), j


class Rig(object):
    """a context, the frames in its slots as the composition wants them, and the call on both sides"""

    def __init__(self, hip_lib, levels):
        self.ctx = make_ctx(hip_lib, width=W, height=H, levels=levels, max_frames=10)
        self.levels, self.frames = levels, {}
        self.src = sr.texture(W + SHIFT * 8, H, 5)
        px, level = sr.lattice(W + SHIFT * 8, H, 12)
        order = np.random.default_rng(9).permutation(len(level))
        self.lat_px, self.lat_level = px[order], (level[order] % levels).astype(np.int32)
        self.lat_angle = np.random.default_rng(10).uniform(0, 360, len(level)).astype(np.float32)
        self.ready = False

    def put(self, slot, k, n=None, depth=None, has_mp=None, px=None, level=None, angle=None, seed=0):
        """frame k of the sequence into `slot` with its first n lattice keypoints (all that lie inside the picture when n is None)"""
        rng = np.random.default_rng(1000 + 17 * slot + seed)
        self.ctx.upload_gray(slot, np.ascontiguousarray(self.src[:, k * SHIFT:k * SHIFT + W]))
        self.ctx.build_pyramid(slot, 1)
        if px is None:
            x = self.lat_px[:, 0] - k * SHIFT
            keep = np.flatnonzero((x >= 12) & (x <= W - 12))[:n]
            px, level, angle = np.stack([x[keep], self.lat_px[keep, 1]], 1), self.lat_level[keep], self.lat_angle[keep]
        m = len(level)
        assert n is None or m == n
        depth = np.full(m, Z) if depth is None else depth
        has_mp = (rng.uniform(size=m) < 0.6).astype(np.uint8) if has_mp is None else has_mp
        self.ctx.describe_given_angle(slot, px, level, angle)
        self.ctx.set_keypoint_depths(slot, np.asarray(depth, np.float64), np.asarray(has_mp, np.uint8))
        kp = self.ctx.get_keypoints_batch(slot, 1)
        cnt = int(kp["count"][0])
        d, hm = self.ctx.get_keypoint_depths(slot)
        assert cnt == m and len(d) == m
        self.frames[slot] = dict(px=kp["px"][0, :cnt].copy(), level=kp["level"][0, :cnt].copy(), desc=kp["desc"][0, :cnt].copy(), depth=d, has_mp=hm)
        return self.frames[slot]

    def sequence(self):
        if not self.ready:
            for k in range(6):
                self.put(k, k)
            self.ready = True

    def prior_rows(self, priors):
        """[n, cells] from a list of None / arrays by keypoint"""
        out = np.full((len(priors), self.ctx.cells), -1, np.int32)
        for f, p in enumerate(priors):
            if p is not None:
                out[f, :len(p)] = p
        return out

    def both(self, sets, slots, set_index, T, prior=None, pose=None, **kw):
        fields = dict(kw)
        if pose:
            fields.update({"pose_" + k: v for k, v in pose.items()})
        rows = None if prior is None else self.prior_rows(prior)
        got = self.ctx.stereo_local_map_slots(sets, slots, set_index, T, rows, **fields)
        want = sl.local_map(self.frames, sets, slots, set_index, T, prior, cells=self.ctx.cells, K=K, w=W, h=H, L=self.levels,
                            pose=None if pose is None else sl.pose_params(kw.get("baseline", 0.1), **pose), **kw)
        same(got, want)
        return got


@pytest.fixture(scope="module")
def rig(hip_lib):
    r = Rig(hip_lib, 3)
    yield r
    r.ctx.close()


@pytest.fixture(scope="module")
def rig1(hip_lib):
    r = Rig(hip_lib, 1)
    yield r
    r.ctx.close()


def test_frames_sharing_one_set_and_a_second_call(rig):
    rig.sequence()
    assert rig.ctx.cells == 768
    s, _ = point_set(rig.frames[0], len(rig.frames[0]["level"]), 1)
    one = rig.both([s], [0], [0], [shifted(0.4)])
    assert one["status"][0] == 0 and one["counts"][0, 6] > 200 and one["inliers"][0] > 100          # the case is about something
    T = np.stack([shifted(0.4), shifted(-SHIFT + 0.3, 0.2), shifted(-2 * SHIFT)])
    got = rig.both([s], [0, 1, 2], [0, 0, 0], T)
    assert (got["status"] == 0).all() and got["counts"][:, 6].min() > 150
    same(frame_slice(got, 0), one)
    again = rig.ctx.stereo_local_map_slots([s], [0, 1, 2], [0, 0, 0], T)
    same(again, got)
    assert np.abs(got["T_out"][:, 4] + np.arange(3) * SHIFT * Z / K[0]).max() < 2e-3               # the pictures move by SHIFT pixels


def test_65_frames_sets_of_different_sizes_and_a_slot_with_two_poses(rig):
    rig.sequence()
    rng = np.random.default_rng(21)
    sets = [point_set(rig.frames[0], 700, 2)[0], point_set(rig.frames[2], 90, 3)[0], dict(), point_set(rig.frames[4], 300, 4, start=50)[0]]
    home = [0, 2, 0, 4]
    slots = [int(rng.integers(0, 6)) for _ in range(65)]
    slots[:2] = [3, 3]                                                   # the same slot twice with two poses
    st = [int(rng.integers(0, 4)) for _ in range(65)]
    T = np.stack([shifted(-(sl_ - home[s_]) * SHIFT + rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)) for sl_, s_ in zip(slots, st)])
    prior = []
    for f in range(65):
        n_kp, n_pt = len(rig.frames[slots[f]]["level"]), strack_ref.set_size(sets[st[f]])
        p = np.full(n_kp, -1, np.int32)
        if n_pt and f % 3:
            who = rng.choice(n_kp, min(n_kp, 40), replace=False)
            p[who] = rng.integers(0, n_pt, len(who))
        prior.append(p)
    got = rig.both(sets, slots, st, T, prior)
    assert (got["status"] == 0).sum() > 30 and (got["status"] == 1).sum() >= 1 and len(set(zip(slots, st))) > 15
    assert got["T_out"][0].tobytes() != got["T_out"][1].tobytes()


@pytest.mark.parametrize("k", range(len(PT_SIZES)))
def test_wavefront_and_tile_edges(rig, k):
    rig.sequence()
    n_pt, n_kp = PT_SIZES[k], KP_SIZES[k % len(KP_SIZES)]
    rig.put(6, 0, n=n_kp)
    small, full = point_set(rig.frames[0], n_pt, 10 + k)[0], point_set(rig.frames[0], len(rig.frames[0]["level"]), 5)[0]
    few = point_set(rig.frames[6], n_pt, 30 + k)[0]
    got = rig.both([small, full, few], [0, 6, 6, 1], [0, 1, 2, 0], np.stack([shifted(0.3), shifted(0.0, 0.4), shifted(0.2), shifted(-SHIFT)]),
                   min_edges=1, pose=dict(min_edges=1))
    assert got["counts"][:, 0].tolist() == [len(rig.frames[0]["level"]), n_kp, n_kp, len(rig.frames[1]["level"])]
    assert got["counts"][:, 3].tolist() == [n_pt, len(rig.frames[0]["level"]), n_pt, n_pt] and got["counts"][:, 6].sum() > 1


@pytest.mark.parametrize("n", (64, 257))
def test_single_level_pyramid(rig1, n):
    rig1.put(0, 0)
    rig1.put(1, 1)
    rig1.put(2, 0, n=n)
    s = point_set(rig1.frames[0], 600, 6)[0]
    got = rig1.both([s], [0, 1, 2], [0, 0, 0], np.stack([shifted(0.2), shifted(-SHIFT), shifted(0.0)]))
    assert got["counts"][0, 6] > 100


def test_priors_none_partial_all_taken_and_duplicates(rig):
    rig.sequence()
    fr = rig.frames[0]
    n = len(fr["level"])
    s, j = point_set(fr, n + 200, 7)
    T = np.tile(shifted(0.3), (4, 1))
    partial = np.full(n, -1, np.int32)
    partial[::2] = np.arange(n)[::2]                                      # point i sits on keypoint i
    taken = np.arange(n, dtype=np.int32)
    dup = np.full(n, -1, np.int32)
    dup[:60] = np.repeat(np.arange(30), 2)                                # keypoints 2 i and 2 i + 1 both name point i
    got = rig.both([s], [0, 0, 0, 0], [0, 0, 0, 0], T, [None, partial, taken, dup])
    c = got["counts"]
    assert c[0, 2] == 0 and c[1, 2] == (n + 1) // 2 and c[2, 2] == n and c[3, 2] == 60
    assert c[2, 6] == 0 and c[2, 7] == n and (got["outcome"][got["offsets"][2]:got["offsets"][3]] <= strack_ref.NO_CANDIDATE).all()
    assert c[1, 6] > 50 and np.array_equal(got["kp_point"][3, :60], dup[:60])
    same(frame_slice(got, 0), rig.both([s], [0], [0], T[:1]))               # a NULL prior array is the all-free prior
    same(frame_slice(got, 2), rig.both([s], [0], [0], T[:1], [taken]))


def craft(a, b, da, db_minus_da, rng):
    """a descriptor da + y bits from a and db_minus_da further from b, for two descriptors a, b; (desc, its distance to a, to b)"""
    A, B = np.unpackbits(a), np.unpackbits(b)
    diff, eq = np.flatnonzero(A != B), np.flatnonzero(A == B)
    x = max((len(diff) - db_minus_da) // 2, 0)
    y = max(da - x, 0)
    d = A.copy()
    d[rng.choice(diff, x, replace=False)] ^= 1
    d[rng.choice(eq, y, replace=False)] ^= 1
    return np.packbits(d), x + y, len(diff) - x + y


def crafted(rig):
    """slot 7: pairs of level-0 keypoints 2 px apart on a 30 px grid.  Set A has one point between the two of every pair, its descriptor a
    little nearer to the first: the ratio rule fires.  Set B has three points on every first keypoint: contention.  Set C holds two points."""
    px = np.array([(x + dx, y) for y in range(30, H - 30, 30) for x in range(30, W - 30, 30) for dx in (0.0, 2.0)])
    m = len(px)
    rng = np.random.default_rng(77)
    fr = rig.put(7, 0, px=px, level=np.zeros(m, np.int32), angle=rng.uniform(0, 360, m).astype(np.float32), has_mp=np.ones(m, np.uint8))
    first = np.arange(0, m, 2)
    mid = fr["px"][first] + [1.0, 0.0]
    Pc = np.stack([(mid[:, 0] - K[2]) / K[0] * Z, (mid[:, 1] - K[3]) / K[1] * Z, np.full(len(mid), Z)], 1)
    d = np.linalg.norm(Pc, axis=1)
    made = [craft(fr["desc"][i], fr["desc"][i + 1], 0, 10 if (i // 2) % 2 == 0 else 60, rng) for i in first]
    A = dict(pw=Pc, pt_desc=np.stack([q[0] for q in made]), pt_dmax=0.9 * d, pt_normal=Pc / d[:, None])
    fires = np.array([q[1] <= 100 and q[1] > 0.8 * q[2] for q in made])
    rep = np.repeat(np.arange(len(first)), 3)
    B = dict(pw=Pc[rep] + np.tile([[0.0, 0, 0], [0.002, 0, 0], [0, 0.002, 0]], (len(first), 1)),
             pt_desc=np.stack([proj_ref.flip_bits(rng, fr["desc"][first[i]], int(rng.integers(0, 30))) for i in rep]), pt_dmax=0.9 * d[rep],
             pt_normal=(Pc / d[:, None])[rep])
    C = {k: v[np.flatnonzero(~fires)[:2]] for k, v in A.items()}
    return A, B, C, fires


def test_crafted_frames_alone_and_beside_others(rig):
    rig.sequence()
    A, B, C, fires = crafted(rig)
    n0 = len(rig.frames[0]["level"])
    full, _ = point_set(rig.frames[0], n0, 8)
    hundred = np.full(n0, -1, np.int32)
    hundred[:100] = np.arange(100)
    fifty = point_set(rig.frames[0], 50, 9, bits=0, start=100)[0]
    p50 = np.full(n0, -1, np.int32)
    p50[100:150] = np.arange(50)
    sets = [full, A, B, C, fifty]
    slots, st = [1, 0, 7, 7, 7, 0, 2], [0, 0, 1, 2, 3, 4, 0]
    T = np.stack([shifted(-SHIFT), shifted(0.3), shifted(0.0), shifted(0.0), shifted(0.1), shifted(0.2), shifted(-2 * SHIFT)])
    prior = [None, hundred, None, None, None, p50, None]
    got = rig.both(sets, slots, st, T, prior, th_dist=100)
    o = lambda f, k: got[k][got["offsets"][f]:got["offsets"][f + 1]]
    assert got["counts"][1, 2] == 100 and (o(1, "reason")[:100] == strack_ref.SKIP).all() and got["counts"][1, 7] >= 100
    assert np.array_equal(got["kp_point"][1, :100], np.arange(100))
    assert fires.sum() > 5 and (~fires).sum() > 5 and np.array_equal(o(2, "outcome") == strack_ref.RATIO, fires)      # the ratio rule, no claim
    assert (o(2, "match")[fires] == -1).all() and (o(2, "match")[~fires] >= 0).all()
    # contention: three points on every pair of keypoints, so at least one of the three stays without a keypoint
    assert got["counts"][3, 3] == 3 * len(fires) and len(fires) <= got["counts"][3, 6] <= 2 * len(fires)
    assert (o(3, "outcome") > strack_ref.MATCHED).sum() >= len(fires) and (o(3, "match") >= 0).sum() == got["counts"][3, 6]
    assert got["status"][4] == 1 and got["counts"][4, 7] == 2 and got["T_out"][4].tobytes() == T[4].tobytes()          # two edges
    assert not got["outlier"][4].any() and (got["chi2"][4] == -1.0).all() and got["round_status"][4, 0] == popt_ref.FAILED
    assert got["counts"][5].tolist()[2:] == [50, 50, 0, 0, 0, 50] and got["status"][5] == 0 and got["inliers"][5] > 20  # the prior alone
    assert got["status"][0] == 0 and got["status"][6] == 0
    for f in (1, 2, 3, 4, 5):
        alone = rig.both([sets[st[f]]], [slots[f]], [0], T[f:f + 1], None if prior[f] is None else [prior[f]], th_dist=100)
        same(alone, frame_slice(got, f))


def test_empty_set(rig):
    rig.sequence()
    full, _ = point_set(rig.frames[0], 300, 8)
    got = rig.both([dict(), full], [0, 0, 1], [0, 1, 0], np.stack([shifted(0.3), shifted(0.3), shifted(0.0)]))
    assert got["offsets"].tolist() == [0, 0, 300, 300] and got["status"].tolist() == [1, 0, 1] and (got["kp_point"][0] == -1).all()
    assert got["T_out"][0].tobytes() == shifted(0.3).tobytes()
    only = rig.both([dict()], [0, 1], [0, 0], np.stack([shifted(0.3), shifted(0.0)]))       # nothing to search in the whole call
    assert len(only["match"]) == 0 and (only["status"] == 1).all()


def test_overflow_more_than_eight_candidates(rig):
    px = np.array([(x, y) for y in range(20, H - 20, 2) for x in range(20, W - 20, 6)], np.float64)[:760]
    fr = rig.put(8, 1, px=px, level=np.zeros(len(px), np.int32), angle=np.zeros(len(px), np.float32))
    s, _ = point_set(fr, 200, 11, start=300)
    s["pt_dmax"] = s["pt_dmax"] * 2.0                                      # predicted level 1: a window of 5 px (10 with r_wide)
    got = rig.both([s], [8], [0], [shifted(0.0)], th_dist=256, cos_near=2.0)
    assert got["counts"][0, 5] > 20 and (got["n_cand"] > 8).sum() == got["counts"][0, 5]
    rig.both([s], [8], [0], [shifted(0.0)])


def test_mono_keypoints(rig):
    """a keypoint whose u - bf / depth is negative counts as mono; a flag of 0 with a depth, and a NaN depth, have no depth"""
    rig.sequence()
    n = len(rig.frames[0]["level"])
    dc, hc = np.full(n, Z), np.ones(n, np.uint8)
    dc[::4] = 0.05                                                       # bf / 0.05 = 1042 pixels: the right column is far below zero
    dc[1::7] = np.nan
    hc[2::7] = 0
    fr = rig.put(6, 0, depth=dc, has_mp=hc)
    s, _ = point_set(fr, n, 12)
    prior = np.full(n, -1, np.int32)
    prior[:20] = np.arange(20)                                           # keypoints 0, 4, ... of them are mono: prior edges of kind 1
    got = rig.both([s], [6], [0], [shifted(0.3)], [prior])
    ur = sl.right_columns(fr["px"], fr["depth"], sl.has_depth(fr["depth"], fr["has_mp"]), 0.1, K)
    near = (fr["depth"] == 0.05) & (fr["has_mp"] != 0)
    assert near.sum() > 50 and (ur[near] < -100).all() and got["counts"][0, 1] == (ur >= 0).sum() < n - near.sum()
    mono = np.flatnonzero((ur < 0) & (got["kp_point"][0, :n] >= 0))
    assert len(mono) > 30 and got["counts"][0, 6] > 100                  # they are matched and went into the optimiser as mono edges


@pytest.mark.parametrize("fields,pose", [(dict(th=3.0), None), (dict(th_dist=50), None), (dict(ratio=1.0), None), (dict(min_edges=0), None),
                                         (dict(min_edges=1000), None), (dict(), dict(rounds=1)),
                                         (dict(baseline=0.3, r_near=1.5, r_wide=2.0, cos_near=0.9), dict(min_rel_decrease=1e-6, robust_rounds=1))])
def test_other_parameters(rig, fields, pose):
    rig.sequence()
    s, _ = point_set(rig.frames[0], 900, 13, bits=70)
    prior = np.full(len(rig.frames[1]["level"]), -1, np.int32)
    prior[5:25] = np.arange(20)
    got = rig.both([s, dict()], [0, 1, 1], [0, 0, 1], np.stack([shifted(1.0), shifted(-SHIFT + 0.5), shifted(0.0)]), [None, prior, None],
                   pose=pose, **fields)
    if fields.get("min_edges") == 1000:
        assert (got["status"] == 1).all() and (got["T_out"][0] == shifted(1.0)).all() and got["counts"][0, 7] > 100
    if fields.get("min_edges") == 0:
        assert (got["status"] == 0).all() and got["counts"][2, 7] == 0
    if pose and pose.get("rounds") == 1:
        assert (got["rounds_run"] == 1).all()


def test_errors_through_a_live_context(rig, hip_lib):
    rig.sequence()
    E, ctx = hip_lib.YgzHipError, rig.ctx
    s, _ = point_set(rig.frames[0], 64, 14)
    I = sl.IDENTITY

    def code(*a, **kw):
        with pytest.raises(E) as e:
            ctx.stereo_local_map_slots(*a, **kw)
        return e.value.code
    n = hip_lib.SLM_MAX_FRAMES + 1
    assert code([s], [0] * n, [0] * n, np.tile(I, (n, 1)), outputs=False) == hip_lib.E_CAPACITY
    ok = ctx.stereo_local_map_slots([s], [0] * (n - 1), [0] * (n - 1), np.tile(I, (n - 1, 1)), outputs=False)
    assert (ok["status"] == ok["status"][0]).all() and (ok["T_out"] == ok["T_out"][0]).all()
    m = hip_lib.SLM_MAX_SETS + 1
    assert code([s] * m, [0], [0], [I], outputs=False) == hip_lib.E_CAPACITY
    assert ctx.stereo_local_map_slots([s] * (m - 1), [0], [m - 2], [I], outputs=False)["status"][0] == ok["status"][0]
    big, _ = point_set(rig.frames[0], hip_lib.SLM_MAX_PAIRS // 1024 + 1, 15, bits=0)
    assert code([big], [0] * 1024, [0] * 1024, np.tile(I, (1024, 1)), outputs=False) == hip_lib.E_CAPACITY
    at = {k: v[:-1] for k, v in big.items()}                              # the limit itself: 1024 frames of 4096 points
    lim = ctx.stereo_local_map_slots([at], [0] * 1024, [0] * 1024, np.tile(I, (1024, 1)), outputs=False)
    assert (lim["T_out"] == lim["T_out"][0]).all() and (lim["status"] == 0).all()
    assert code([s], [10], [0], [I]) == hip_lib.E_INVALID and code([s], [-1], [0], [I]) == hip_lib.E_INVALID
    assert code([s], [0], [1], [I]) == hip_lib.E_INVALID and code([s], [0], [-1], [I]) == hip_lib.E_INVALID
    assert code([s], [], [], np.zeros((0, 7))) == hip_lib.E_INVALID and code([], [0], [0], [I]) == hip_lib.E_INVALID
    bad = I.copy()
    bad[5] = np.inf
    assert code([s], [0], [0], [bad]) == hip_lib.E_INVALID
    nan = dict(s, pw=s["pw"].copy())
    nan["pw"][3, 1] = np.nan
    assert code([nan], [0], [0], [I]) == hip_lib.E_INVALID
    rows = np.full((1, ctx.cells), -1, np.int32)
    for v, at_ in ((64, 0), (-2, 5), (0, ctx.cells - 1)):
        r = rows.copy()
        r[0, at_] = v
        if v == 0:
            ctx.stereo_local_map_slots([s], [0], [0], [I], r)            # in range: accepted, also past the last keypoint
        else:
            assert code([s], [0], [0], [I], r) == hip_lib.E_INVALID, v
    assert code([dict()], [0], [0], [I], np.zeros((1, ctx.cells), np.int32)) == hip_lib.E_INVALID     # no point to name
    for f in (dict(baseline=0.0), dict(th=0.0), dict(th=np.nan), dict(th_dist=257), dict(th_dist=-1), dict(ratio=0.0), dict(r_near=0.0),
              dict(r_wide=-1.0), dict(cos_near=np.nan), dict(min_edges=-1), dict(pose_rounds=0), dict(pose_rounds=9), dict(pose_iterations=65),
              dict(pose_max_trials=0), dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=np.inf)):
        assert code([s], [0], [0], [I], **f) == hip_lib.E_INVALID, f
    assert code([s], [FREE], [0], [I]) == hip_lib.E_STATE and code([s], [0, FREE], [0, 0], [I, I]) == hip_lib.E_STATE
    rig.both([s], [0], [0], [shifted(0.2)])                               # the context is none the worse for it


def test_state_error_without_depths(hip_lib):
    ctx = make_ctx(hip_lib, width=W, height=H, levels=3, max_frames=2)
    try:
        ctx.upload_gray(0, sr.texture(W, H, 5))
        ctx.build_pyramid(0, 1)
        s = dict(pw=np.array([[0.0, 0, 4]]), pt_desc=np.zeros((1, 32), np.uint8), pt_dmax=np.array([4.0]), pt_normal=np.array([[0.0, 0, 1]]))
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.stereo_local_map_slots([s], [0], [0], [sl.IDENTITY])
        assert e.value.code == hip_lib.E_STATE
    finally:
        ctx.close()
