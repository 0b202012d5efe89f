"""Stereo odometry on resident slots on the MI355X (ygz_slam_amd/csrc/svo.hip: k_svo_gather, k_svo_resolve, k_svo_scatter around k_strack_search
and k_pose_opt) against the composition tests/svo_ref.py: EVERY output of EVERY pair is bit-identical to the composition run on the arrays
fetched from the same slots (get_keypoints_batch, get_keypoint_depths), doubles compared as their 64 bits.

One QVGA context with 3 levels and 10 slots (768 cells) and one with a single level.  The pictures are windows of one texture that move by 3
pixels per frame; the keypoints are hand-placed lattice points that move with it (describe_given_angle), 60 % of them with the constant depth
of the scene (set_keypoint_depths), so the matches and the edges are real.  No case is left out of the comparison."""
import numpy as np
import pytest

import popt_ref
import stereo_ref as sr
import strack_ref
import svo_ref as sv
from conftest import make_ctx

pytestmark = pytest.mark.gpu

W, H, SHIFT, Z = 320, 240, 3, 4.0
K = popt_ref.DEFAULT_K
SIZES = (1, 63, 64, 65, 255, 256, 257)
DOUBLES = ("T_rel", "proj", "chi2", "cost_initial", "cost_final", "lambda")
INTS = ("status", "counts", "rot", "outlier", "inliers", "rounds_run", "round_status", "lm_iterations") + sv.INT_OUTPUTS
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

    def lattice_in(self, k, n=None):
        """the lattice keypoints inside frame k, the first n of them: (px, level, angle)"""
        x = self.lat_px[:, 0] - k * SHIFT
        keep = np.flatnonzero((x >= 12) & (x <= W - 12))[:n]
        return np.stack([x[keep], self.lat_px[keep, 1]], 1), self.lat_level[keep], self.lat_angle[keep]

    def put(self, slot, k, n=None, depth=None, has_mp=None, angle=None, px=None, level=None, seed=0):
        """frame k of the sequence into `slot` with its first n lattice keypoints (all that lie inside the picture when n is None)"""
        rng = np.random.default_rng(1000 + 17 * slot + seed)
        self.ctx.upload_gray(slot, np.ascontiguousarray(self.src[:, k * SHIFT:k * SHIFT + W]))
        self.ctx.build_pyramid(slot, 1)
        if px is None:
            x = self.lat_px[:, 0] - k * SHIFT
            keep = np.flatnonzero((x >= 12) & (x <= W - 12))[:n]
            px, level = np.stack([x[keep], self.lat_px[keep, 1]], 1), self.lat_level[keep]
            angle = self.lat_angle[keep] if angle is None else np.asarray(angle, np.float32)[keep]
        m = len(level)
        assert n is None or m == n
        if depth is None:
            depth = np.full(m, Z)
        if has_mp is None:
            has_mp = (rng.uniform(size=m) < 0.6).astype(np.uint8)
        self.ctx.describe_given_angle(slot, px, level, angle)
        self.ctx.set_keypoint_depths(slot, np.asarray(depth, np.float64), np.asarray(has_mp, np.uint8))
        kp = self.ctx.get_keypoints_batch(slot, 1)
        cnt = int(kp["count"][0])
        d, hm = self.ctx.get_keypoint_depths(slot)
        assert cnt == m and len(d) == m
        self.frames[slot] = dict(px=kp["px"][0, :cnt].copy(), level=kp["level"][0, :cnt].copy(), angle=kp["angle"][0, :cnt].copy(),
                                 desc=kp["desc"][0, :cnt].copy(), depth=d, has_mp=hm)
        return self.frames[slot]

    def sequence(self):
        for k in range(6):
            self.put(k, k)

    def both(self, last, cur, T_init=None, direction=None, pose=None, **kw):
        fields = dict(kw)
        if pose:
            fields.update({"pose_" + k: v for k, v in pose.items()})
        got = self.ctx.stereo_odometry_slots(last, cur, T_init, direction, **fields)
        want = sv.odometry(self.frames, last, cur, self.ctx.cells, T_init, direction, K=K, w=W, h=H, L=self.levels,
                           pose=None if pose is None else sv.pose_params(kw.get("baseline", 0.1), **pose), **kw)
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


def shifted_guess(pixels):
    """the last camera -> current camera pose that moves the projections of the scene's depth by `pixels` along x"""
    return np.array([0, 0, 0, 1.0, pixels * Z / K[0], 0, 0])


def test_chain_of_pairs_and_a_second_call(rig):
    rig.sequence()
    assert rig.ctx.cells == 768
    one = rig.both([0], [1])
    assert one["status"][0] == 0 and one["counts"][0, 3] > 100 and one["inliers"][0] > 50           # the case is about something
    # frame k is the current frame of pair k - 1 and the last frame of pair k
    got = rig.both([0, 1, 2], [1, 2, 3])
    assert (got["status"] == 0).all()
    same({k: v[:1] for k, v in got.items()}, one)
    again = rig.ctx.stereo_odometry_slots([0, 1, 2], [1, 2, 3])
    same(again, got)
    # the pictures move by SHIFT pixels: the pose says so
    assert np.abs(got["T_rel"][:, 4] + SHIFT * Z / K[0]).max() < 2e-3


def test_65_pairs_in_one_call(rig):
    rig.sequence()
    rng = np.random.default_rng(21)
    last = [k % 5 for k in range(65)]
    cur = [(k % 5) + 1 if k % 3 else (k + 2) % 6 for k in range(65)]
    last = [l if l != c else (c + 3) % 6 for l, c in zip(last, cur)]
    T = np.tile(sv.IDENTITY, (65, 1))
    T[:, 4] = rng.uniform(-0.03, 0.03, 65)
    T[::4, 6] = rng.choice([-0.25, 0.25], len(T[::4]))                  # derived directions of either sign
    got = rig.both(last, cur, T)
    assert (got["status"] == 0).sum() > 30 and len(set(zip(last, cur))) > 10


@pytest.mark.parametrize("n", SIZES)
def test_wavefront_and_tile_edges(rig, n):
    rig.sequence()
    rig.put(6, 0, n=n)
    rig.put(7, 1, n=n)
    got = rig.both([6, 0, 6], [1, 7, 7], min_matches=1 if n == 1 else 20)
    assert got["counts"][:, 0].tolist() == [n, rig.frames[0]["level"].size, n] and got["counts"][:, 2].tolist() == [rig.frames[1]["level"].size, n, n]


@pytest.mark.parametrize("n", (64, 257))
def test_single_level_pyramid(rig1, n):
    rig1.put(0, 0)
    rig1.put(1, 1)
    rig1.put(2, 0, n=n)
    got = rig1.both([0, 2, 1], [1, 1, 2], direction=[0, 1, -1])
    assert got["counts"][0, 3] > 100


@pytest.mark.parametrize("direction", (-1, 0, 1, None))
def test_directions_given_and_derived(rig, direction):
    rig.sequence()
    T = np.tile(sv.IDENTITY, (3, 1))
    T[:, 6] = [-0.25, 0.0, 0.25]                                        # derived: +1, 0, -1
    got = rig.both([0, 1, 2], [1, 2, 3], T, None if direction is None else [direction] * 3)
    if direction is None:
        want = [strack_ref.direction(sv.IDENTITY, t, 0.1) for t in T]
        assert want == [1, 0, -1]
    assert got["counts"][:, 4].min() > 50


def test_crafted_pairs_alone_and_beside_others(rig):
    rig.sequence()
    rig.put(6, 0, n=5, has_mp=np.ones(5, np.uint8))                      # too few matches
    rig.put(7, 0, has_mp=np.zeros(rig.frames[0]["level"].size, np.uint8))   # a last frame without any depth
    # the retry that succeeds: level-0 points whose projections are 10 pixels off, outside th = 7 and inside 14; 10 pixels off is 2 pixels
    # from the lattice neighbour, which th_dist = 50 keeps out
    px, _, angle = rig.lattice_in(0)
    rig.put(8, 0, px=px, level=np.zeros(len(px), np.int32), angle=angle, has_mp=np.ones(len(px), np.uint8))
    T = np.stack([shifted_guess(-SHIFT - 10.0), sv.IDENTITY, sv.IDENTITY, sv.IDENTITY, shifted_guess(2.0)])
    got = rig.both([8, 6, 7, 2, 1], [1, 1, 1, 3, 2], T, th_dist=50)
    assert got["counts"][0, 7] == 1 and got["status"][0] == 0 and got["counts"][0, 3] >= 20         # the retry succeeds
    assert got["status"][1] == 1 and got["counts"][1, 7] == 1 and 0 < got["counts"][1, 3] < 20 and got["T_rel"][1].tobytes() == T[1].tobytes()
    assert got["round_status"][1, 0] == popt_ref.FAILED and not got["outlier"][1].any() and (got["chi2"][1] == -1.0).all()
    assert got["status"][2] == 1 and got["counts"][2, 1] == 0 and got["counts"][2, 4] == 0 and (got["reason"][2, :5] == strack_ref.SKIP).all()
    assert got["status"][3] == 0 and got["status"][4] == 0 and got["counts"][3, 7] == 0
    for p, (l, c) in enumerate([(8, 1), (6, 1), (7, 1)]):
        alone = rig.both([l], [c], T[p:p + 1], th_dist=50)
        same(alone, {k: v[p:p + 1] for k, v in got.items()})


def test_contention_more_points_than_keypoints(rig):
    """every keypoint of the current frame is wanted by three points of the last one: the walk's taken chain decides"""
    cur = rig.put(1, 1, n=80, has_mp=np.ones(80, np.uint8))
    px = np.repeat(cur["px"] + [SHIFT, 0], 3, axis=0) + np.tile([[0.0, 0], [1, 0], [0, 1]], (80, 1))
    rig.put(6, 0, px=px, level=np.repeat(cur["level"], 3), angle=np.repeat(cur["angle"], 3), has_mp=np.ones(240, np.uint8))
    got = rig.both([6], [1], th_dist=256, check_orientation=0)
    oc = got["outcome"][0, :240]
    assert got["counts"][0, 0] == 240 and got["counts"][0, 2] == 80 and (oc == strack_ref.NO_CANDIDATE).sum() + (got["dist"][0, :240] > 0).sum() > 40
    rig.both([6], [1])
    rig.put(1, 1)


def test_overflow_more_than_eight_candidates(rig):
    px = np.array([(x, y) for y in range(20, H - 20, 4) for x in range(20, W - 20, 6)], np.float64)[:700]
    rig.put(7, 1, px=px, level=np.full(len(px), 1, np.int32), angle=np.zeros(len(px), np.float32))
    rig.put(6, 0, n=100, has_mp=np.ones(100, np.uint8))
    got = rig.both([6], [7], th_dist=256)
    assert got["counts"][0, 5] > 20 and (got["n_cand"][0, :100] > 8).sum() == got["counts"][0, 5]
    rig.both([6], [7])


def test_orientation_rule_removes_matches(rig):
    turned = (rig.lat_angle + 20).astype(np.float32)
    wild = np.random.default_rng(4).uniform(size=len(turned)) < 1 / 6
    turned[wild] = np.random.default_rng(5).uniform(0, 360, int(wild.sum())).astype(np.float32)
    rig.put(6, 0, angle=np.mod(turned, 360).astype(np.float32))
    rig.put(1, 1)
    got = rig.both([6], [1])
    assert got["counts"][0, 6] > 5 and (got["outcome"][0] == strack_ref.ORIENTATION).sum() == got["counts"][0, 6]
    off = rig.both([6], [1], check_orientation=0)
    assert off["counts"][0, 6] == 0 and off["counts"][0, 3] == got["counts"][0, 3] + got["counts"][0, 6]


def test_depth_rules(rig):
    """a keypoint whose u - bf / depth is negative counts as mono; a flag of 0 with a depth, and a NaN depth, have no depth"""
    rig.put(0, 0)
    n = rig.frames[0]["level"].size
    m = rig.put(1, 1)["level"].size
    dl, hl = np.full(n, Z), np.ones(n, np.uint8)
    dl[::5] = np.nan
    hl[1::5] = 0
    dc, hc = np.full(m, Z), np.ones(m, np.uint8)
    dc[::4] = 0.05                                                       # bf / 0.05 = 1042 pixels: the right column is far below zero
    dc[1::7] = np.nan
    hc[2::7] = 0
    last, cur = rig.put(6, 0, depth=dl, has_mp=hl), rig.put(7, 1, depth=dc, has_mp=hc)
    hd = sv.has_depth(cur["depth"], cur["has_mp"])
    ur = sv.right_columns(cur["px"], cur["depth"], hd, 0.1, K)
    near = np.flatnonzero(hd & (cur["depth"] == 0.05))
    assert len(near) > 50 and (ur[near] < -100).all() and np.isnan(last["depth"][::5]).all()
    got = rig.both([6, 7], [7, 6])
    assert got["counts"][0, 1] == n - len(dl[::5]) - len(hl[1::5]) and (got["reason"][0, :n:5] == strack_ref.SKIP).all()
    assert (got["reason"][0, 1:n:5] == strack_ref.SKIP).all() and got["counts"][0, 3] > 50
    matched_near = [j for j in got["match"][0, :n] if j in set(near.tolist())]
    assert len(matched_near) > 5                                         # they went into the optimiser as mono edges


@pytest.mark.parametrize("fields,pose", [(dict(th=15.0), None), (dict(th_dist=50), None), (dict(check_orientation=0), None),
                                         (dict(min_matches=0), None), (dict(min_matches=1000), None), (dict(), dict(rounds=1)),
                                         (dict(baseline=0.3, th=3.5), dict(min_rel_decrease=1e-6, robust_rounds=1))])
def test_other_parameters(rig, fields, pose):
    rig.sequence()
    got = rig.both([0, 3], [1, 4], np.stack([shifted_guess(1.0), sv.IDENTITY]), pose=pose, **fields)
    if fields.get("min_matches") == 1000:
        assert (got["status"] == 1).all() and (got["counts"][:, 7] == 1).all()
    if pose and pose.get("rounds") == 1:
        assert (got["rounds_run"] == 1).all()


def test_errors_through_a_live_context(rig, hip_lib):
    rig.sequence()
    E, ctx = hip_lib.YgzHipError, rig.ctx

    def code(*a, **kw):
        with pytest.raises(E) as e:
            ctx.stereo_odometry_slots(*a, **kw)
        return e.value.code
    n = hip_lib.SVO_MAX_PAIRS + 1
    assert code([0] * n, [1] * n, outputs=False) == hip_lib.E_CAPACITY
    ok = ctx.stereo_odometry_slots([0] * (n - 1), [1] * (n - 1), outputs=False)
    assert (ok["status"] == ok["status"][0]).all() and (ok["T_rel"] == ok["T_rel"][0]).all()
    assert code([0], [0]) == hip_lib.E_INVALID and code([0], [10]) == hip_lib.E_INVALID and code([-1], [1]) == hip_lib.E_INVALID
    assert code([], []) == hip_lib.E_INVALID
    assert code([0], [1], direction=[2]) == hip_lib.E_INVALID
    bad = sv.IDENTITY.copy()
    bad[5] = np.inf
    assert code([0], [1], T_init=bad) == hip_lib.E_INVALID
    for f in (dict(baseline=0.0), dict(th=0.0), dict(th=np.nan), dict(th_dist=257), dict(th_dist=-1), dict(min_matches=-1), dict(pose_rounds=0),
              dict(pose_rounds=9), dict(pose_iterations=65), dict(pose_max_trials=0), dict(pose_chi2_mono=0.0), dict(pose_chi2_stereo=np.inf)):
        assert code([0], [1], **f) == hip_lib.E_INVALID, f
    assert code([0], [FREE]) == hip_lib.E_STATE and code([FREE], [0]) == hip_lib.E_STATE
    rig.both([0], [1])                                                   # the context is none the worse for it
