"""The launch geometry of k_klt3 and k_find_direct_projection (pytest -m gpu): a pair's grid covers 3 / 8 of the detector's cells per pass
-- cells / 8 point triples for LK, ceil(3 cells / 8 / 64) workgroups of 64 candidates for the direct projection -- and a wavefront walks on
in steps of the grid while points are left.  On a 160 x 120 context with the detector's 10-pixel cells, cells = 12 x 16 = 192: LK gets 24
triples = 72 points per pass, the direct projection two workgroups = 128 candidates.  The counts below sit on both sides of every boundary
of those walks (and of a walk in passes of 64 candidates): the last partial triple, the end of a pass, the first wavefront of the second
and third pass, the capacity.  Everything is compared with the oracle only, at the bars of tests/test_gpu_parity.py: LK status equal and
tracks within 1e-5 relative, the direct projection bit for bit."""
import numpy as np
import pytest
from conftest import make_ctx
from ygz_slam_amd import synth

pytestmark = pytest.mark.gpu
W, H, LEVELS, CELLS = 160, 120, 3, 192
LK_COUNTS = [0, 1, 2, 3, 4, 71, 72, 73, 144, 145, 192]
FDP_COUNTS = [0, 1, 63, 64, 65, 128, 129, 192]


def _dense_frames(n):
    """frames with a corner in nearly every detector cell (a seeded block texture, moved by up to 2 pixels per frame): about 110 keypoints,
    more than one pass of 72"""
    rng = np.random.default_rng(31)
    big = np.kron(rng.integers(0, 2, (H // 4 + 8, W // 4 + 8)).astype(np.uint8) * 160 + 40, np.ones((4, 4), np.uint8))
    big = (big.astype(np.int32) + rng.integers(-8, 9, big.shape)).clip(0, 255).astype(np.uint8)
    return [np.ascontiguousarray(big[(i // 3) % 3:(i // 3) % 3 + H, i % 3:i % 3 + W]) for i in range(n)]


@pytest.fixture(scope="module")
def case(oracle):
    """two seeded synthetic pairs, 192 seeded points / candidates on them and the oracle's answers for all of them, computed once: points
    and candidates are independent, so the answer for the first n is a prefix.
    LK (slots 2 -> 3, the block texture moved by one pixel per axis): the 1e-5 bar is the bar for TRACKED FEATURES -- the reference tracks
    detector corners, and so do the parity tests that set the bar; on a flat patch the normal matrix is near singular and the summation order of
    the mismatch vector (a tree on the GPU) moves the answer by more.  So the points are the 192 FAST corners with the largest Shi-Tomasi
    score, in seeded order, each moved by a seeded sub-pixel offset, and the search starts up to 2 pixels off."""
    tex, m = synth.make_texture(4, W, H, margin=80)
    poses = synth.trajectory(2, 14, 0.4)
    poses[0] = [0, 0, 0, 1, 0, 0, 0]
    ren = [synth.render(tex, m, poses[i], W, H, 1.0, 4000 + i) for i in range(2)]
    imgs, depths = [r[0] for r in ren], [r[1] for r in ren]
    dense = _dense_frames(5)
    imgs += [dense[0], dense[4]]
    rng = np.random.default_rng(23)
    xy = oracle.fast_detect(imgs[2], 15)
    xy = xy[oracle.fast_nonmax(xy, oracle.fast_score(imgs[2], xy, 15), 0)]
    xy = xy[(xy[:, 0] >= 16) & (xy[:, 0] < W - 16) & (xy[:, 1] >= 16) & (xy[:, 1] < H - 16)]
    score = np.array([oracle.shi_tomasi(imgs[2], int(x), int(y)) for x, y in xy])
    xy = xy[np.argsort(-score, kind="stable")[:CELLS]]
    assert len(xy) == CELLS
    pts = (xy[rng.permutation(CELLS)] + rng.uniform(-0.5, 0.5, (CELLS, 2))).astype(np.float32)
    init = pts + rng.uniform(-2, 2, pts.shape).astype(np.float32)
    klt = oracle.klt_track(imgs[2], imgs[3], pts, init)
    px_ref = np.stack([rng.uniform(14, W - 14, CELLS), rng.uniform(14, H - 14, CELLS)], 1)
    depth = depths[0][px_ref[:, 1].astype(int), px_ref[:, 0].astype(int)].astype(np.float64)
    depth[[3, 64, 130]] = -1.0                                 # no depth: not ok, level 0 (in both passes)
    level = rng.integers(0, LEVELS, CELLS).astype(np.int32)
    Tcr = oracle.se3_mul(poses[1], oracle.se3_inv(poses[0]))
    R = synth.quat_to_R(Tcr[:4])
    d = np.abs(depth)
    pc = np.stack([(px_ref[:, 0] - synth.CX) / synth.FX * d, (px_ref[:, 1] - synth.CY) / synth.FY * d, d], 1) @ R.T + Tcr[4:]
    pred = np.stack([synth.FX * pc[:, 0] / pc[:, 2] + synth.CX, synth.FY * pc[:, 1] / pc[:, 2] + synth.CY], 1) + rng.uniform(-2, 2, (CELLS, 2))
    pred[9] = [3.0, 3.0]                                       # at the border
    lv = [oracle.pyramid(im, LEVELS) for im in imgs[:2]]
    fdp = oracle.find_direct_projection_n(lv[0], poses[0], lv[1], poses[1], px_ref, depth, level, pred)
    return dict(imgs=imgs, poses=poses, pts=pts, init=init, klt=klt, px_ref=px_ref, depth=depth, level=level, pred=pred, fdp=fdp)


@pytest.fixture(scope="module")
def ctx(hip_lib, case):
    c = make_ctx(hip_lib, width=W, height=H, levels=LEVELS, max_frames=4)
    for s in range(4):
        c.upload_gray(s, case["imgs"][s])
    c.build_pyramid(0, 4)
    assert c.cells == CELLS                                    # the size arithmetic of this file
    yield c
    c.close()


def _lk_check(got, want, tag):
    out, st, _ = got
    oout, ost, _ = want
    assert len(st) == len(ost), tag
    assert np.array_equal(st, ost), tag
    m = ost.astype(bool)
    assert np.all(np.abs(out[m] - oout[m]).max(1) <= 1e-5 * np.maximum(1.0, np.abs(oout[m]).max(1))), tag


@pytest.mark.parametrize("n", LK_COUNTS)
def test_single_pair_lk_counts(ctx, case, n):
    got = ctx.klt_track(2, 3, case["pts"][:n], case["init"][:n])
    _lk_check(got, tuple(a[:n] for a in case["klt"]), n)
    if n == CELLS:
        assert case["klt"][1].mean() > 0.8                     # the case tracks: the comparison is not between two sets of failures


@pytest.mark.parametrize("n", FDP_COUNTS)
def test_direct_projection_counts(ctx, case, n):
    ok, px, sl = ctx.find_direct_projection(0, case["poses"][0], 1, case["poses"][1], case["px_ref"][:n], case["depth"][:n], case["level"][:n],
                                            case["pred"][:n])
    o_ok, o_px, o_sl = (a[:n] for a in case["fdp"])
    assert len(ok) == n
    assert np.array_equal(ok.astype(bool), o_ok)
    has = case["depth"][:n] >= 0                               # without depth the reference returns before it writes px / level
    assert np.array_equal(sl[has], o_sl[has])
    assert np.array_equal(px[has], o_px[has], equal_nan=True)
    if n == CELLS:
        assert o_ok.mean() > 0.4


def test_batched_lk_pairs_with_different_counts(hip_lib, oracle):
    """eight pairs in one launch whose track sets hold 0, 1, 2, 72, 73, 74 points and the detector's full set (twice): a pair's empty
    wavefronts and another pair's second pass share the launch.  The counts are made with the detector's occupied mask."""
    want = [None, 0, 1, 73, 72, 2, None, 74]                   # None: everything the detector finds
    imgs = _dense_frames(8)
    prm = oracle.default_params(W, H, LEVELS)
    cols = -(-W // prm.cell_size)
    occ = np.zeros((8, CELLS), np.uint8)
    for s, k in enumerate(want):
        if k is None:
            continue
        full = oracle.detect(oracle.pyramid(imgs[s], LEVELS), prm)
        cell = (full["py"].astype(int) // prm.cell_size) * cols + full["px"].astype(int) // prm.cell_size
        assert len(full) >= 74 and len(set(cell)) == len(cell)
        occ[s] = 1
        occ[s, cell[:k]] = 0
    c = make_ctx(hip_lib, width=W, height=H, levels=LEVELS, max_frames=8)
    try:
        for s in range(8):
            c.upload_gray(s, imgs[s])
        c.build_pyramid(0, 8)
        c.detect(0, 8, occupied=occ)
        kps = [c.get_keypoints(s)["px"] for s in range(8)]
        for s, k in enumerate(want):
            assert len(kps[s]) == k if k is not None else len(kps[s]) > 74, (s, len(kps[s]))
            if len(kps[s]):
                c.set_keypoint_depths(s, np.ones(len(kps[s])), np.ones(len(kps[s]), np.uint8))
        ref = list(range(8)); cur = [(s + 1) % 8 for s in range(8)]
        I7 = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (8, 1))
        c.track_begin(cur, ref, I7, I7, predict=False)
        c.track_klt()
        tracked = 0
        for p in range(8):
            pts = kps[ref[p]].astype(np.float32)
            o = oracle.klt_track(imgs[ref[p]], imgs[cur[p]], pts, pts)
            _lk_check(c.track_get_klt(p), o, p)
            tracked += int(o[1].sum())
        assert tracked > 150
    finally:
        c.close()
