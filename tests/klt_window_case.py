"""The fixed input of tests/test_gpu_klt_window_reuse.py (and of tools/make_klt_window_golden.py, which wrote its fixture): small frame
pairs on which a stale or mixed window of k_klt3 would show.  k_klt3 keeps a lane's window of the current image between mismatch
evaluations while the window stays on the same pixels, and three points share a wavefront: the cases make the points of one triple
cross pixel boundaries at different evaluations, finish at different counts, leave the image, or never iterate at all.

  small   160 x 120 (the tracker uses levels 0 .. 2 here: a level is dropped when the next one would not exceed the 21 x 21 window),
          25 points, not a multiple of 3 (one pass of the walk over triples: this frame's grid serves 72 points per pass): points within 12 px of every border (negative window corners), guesses that start outside the image, two identical points in
          one triple, one point on a textureless patch (it fails the eigenvalue test while its neighbours iterate).  Tracked with the
          default tracker, and with max_level = 0 (one level, the guesses' whole shift is iterated at full resolution);
  walk    the small pair with 76 points, not a multiple of 3 either: a second pass of the walk (the test checks that it is one), where
          the kept window of a wavefront's first triple must not reach its second;
  tall    352 x 352, all five levels of the default tracker, 1, 2 and 4 points (wavefronts with idle segments);
  batched the small pair through the resident batched path of the step (track_begin with predicted guesses, track_klt).

Every guess is the reference pixel moved by one of SHIFTS, cycled along the points: the members of a triple start from different offsets."""
import numpy as np

from ygz_slam_amd import synth

W, H = 160, 120
TW, TH = 352, 352
SHIFTS = np.array([(0.0, 0.0), (0.49, -0.49), (1.3, 0.7), (-3.7, 2.2)], np.float32)
FLAT = (60, 40, 100, 80)                       # x0, y0, x1, y1 of the textureless patch (both frames)
WIN = 21


def _pair(w, h, seed, flat=None):
    tex, m = synth.make_texture(seed, w, h, margin=80)
    poses = synth.trajectory(2, 11, 0.25)
    out = [synth.render(tex, m, poses[i], w, h, 1.0, 500 + i) for i in range(2)]
    imgs = [np.ascontiguousarray(im) for im, _ in out]
    if flat:
        for im in imgs:
            im[flat[1]:flat[3], flat[0]:flat[2]] = 128
    return imgs, poses, [d for _, d in out]


def small():
    """(imgs, poses, depths, pts, init) of the 160 x 120 pair"""
    imgs, poses, depths = _pair(W, H, 5, FLAT)
    rng = np.random.default_rng(23)
    pts = np.stack([rng.uniform(24, W - 24, 25), rng.uniform(24, H - 24, 25)], 1).astype(np.float32)
    pts[4] = pts[3]                                                     # identical points inside the triple 3, 4, 5
    pts[7] = [0.5 * (FLAT[0] + FLAT[2]), 0.5 * (FLAT[1] + FLAT[3])]     # the textureless patch, between two iterating neighbours
    pts[9], pts[10], pts[11] = [5.0, 60.25], [154.5, 50.0], [70.5, 4.0]             # within 12 px of the left, right and top border
    pts[13], pts[14] = [90.0, 115.5], [3.25, 3.5]                       # bottom border, top-left corner
    pts[24] = [156.5, 116.0]                                            # bottom-right corner, alone in the last triple
    init = pts + SHIFTS[np.arange(25) % 4]
    init[4] = init[3]
    pts[15] = [118.0, 33.5]; init[15] = pts[15] + [-3.7, 2.2]
    init[18] = [-14.0, pts[18][1]]                                      # guesses outside the image: the window is gone at level 0 at the latest
    init[21] = [pts[21][0], H + 13.0]
    pts[19] = [8.0, 30.0]; init[19] = [-4.0, 30.0]                      # starts with the corner at x = -14 and is pulled back
    return imgs, poses, depths, pts, init.astype(np.float32)


# Candidates of walk() that are left out: their tracks wander until the iteration limit stops them (the oracle's iteration tap shows it), or
# stop one iteration apart from the oracle's on the build the fixture was written with.  Such a track amplifies the last bit of a float sum
# (sequential in the oracle, a tree on the GPU) to more than the 1e-5 that the comparison with the oracle allows.
WALK_LEFT_OUT = (2, 23, 25, 31, 37, 43, 62, 71)


def walk():
    rng = np.random.default_rng(29)
    pts = np.stack([rng.uniform(4, W - 4, 80), rng.uniform(4, H - 4, 80)], 1).astype(np.float32)
    more = np.stack([rng.uniform(4, W - 4, 20), rng.uniform(4, H - 4, 20)], 1).astype(np.float32)
    pts = np.concatenate([pts, more])
    init = pts + SHIFTS[np.arange(len(pts)) % 4]
    keep = np.setdiff1d(np.arange(len(pts)), WALK_LEFT_OUT)[:76]
    return pts[keep], init[keep].astype(np.float32)


def tall():
    imgs, poses, depths = _pair(TW, TH, 6)
    pts = np.array([[100.5, 120.25], [30.0, 300.5], [340.0, 20.5], [176.0, 176.0]], np.float32)
    return imgs, pts, (pts + SHIFTS[[1, 2, 3, 0]]).astype(np.float32)


def points_per_pass(cells):
    """of one pair in k_klt3's launch: 3 points per wavefront, 4 wavefronts per workgroup, ceil(ceil(cells / 8) / 4) workgroups"""
    return 3 * 4 * -(-(-(-cells // 8)) // 4)


def put(out, tag, res):
    pts, st, err = res
    out[tag + "pts"] = np.asarray(pts, np.float32)
    out[tag + "status"] = np.asarray(st, np.uint8)
    out[tag + "err"] = np.asarray(err, np.float32)


def track(lib):
    """{"<case>_{pts,status,err}": array}, and the number of grid cells of the small context"""
    out = {}
    imgs, poses, depths, pts, init = small()
    ctx = lib.HipContext(width=W, height=H, levels=3, max_frames=2)
    try:
        cells = ctx.cells
        for s in range(2):
            ctx.upload_gray(s, imgs[s])
        ctx.build_pyramid(0, 2)
        put(out, "small_", ctx.klt_track(0, 1, pts, init))
        prm = ctx.klt_params()
        prm.max_level = 0
        put(out, "level0_", ctx.klt_track(0, 1, pts, init, prm))
        put(out, "walk_", ctx.klt_track(0, 1, *walk()))
        ctx.detect(0, 2)
        for s in range(2):
            px = ctx.get_keypoints(s)["px"]
            d = depths[s][px[:, 1].astype(np.int64), px[:, 0].astype(np.int64)]
            ctx.set_keypoint_depths(s, d, np.ones(len(d), np.uint8))
        ctx.track_begin([1], [0], poses[[1]], poses[[0]], predict=True)
        ctx.track_klt()
        put(out, "batched_", ctx.track_get_klt(0))
    finally:
        ctx.close()
    timgs, tpts, tinit = tall()
    ctx = lib.HipContext(width=TW, height=TH, levels=3, max_frames=2)
    try:
        for s in range(2):
            ctx.upload_gray(s, timgs[s])
        ctx.build_pyramid(0, 2)
        for n in (1, 2, 4):
            put(out, "tall%d_" % n, ctx.klt_track(0, 1, tpts[:n], tinit[:n]))
    finally:
        ctx.close()
    return out, cells


def level0_windows(oracle, imgs, pts, init):
    """The window corners (floor of the position minus half the window) of every evaluation of the one-level track, from the oracle alone:
    a track cut off after k iterations returns the position that evaluation k + 1 starts from.  Returns (corner[k, i, 2] of the
    evaluation k = 0 .., iterating[k, i]): a point iterates at k while cutting it off there still changes its result."""
    prm = oracle.klt_params()
    prm.max_level = 0
    full = oracle.klt_track(imgs[0], imgs[1], pts, init, prm)[0]
    pos = [init.copy()]
    for k in range(1, prm.max_iter):
        prm_k = oracle.klt_params()
        prm_k.max_level = 0
        prm_k.max_iter = k
        pos.append(oracle.klt_track(imgs[0], imgs[1], pts, init, prm_k)[0])
    pos = np.stack(pos)
    half = np.float32((WIN - 1) * 0.5)
    corner = np.floor(pos - half).astype(np.int64)
    inside = (corner[..., 0] >= -WIN) & (corner[..., 0] < W) & (corner[..., 1] >= -WIN) & (corner[..., 1] < H)
    iterating = np.any(pos.view(np.uint32) != full.view(np.uint32)[None], axis=2) & inside
    return corner, iterating


def mixed_evaluations(corner, iterating):
    """per triple of points (as k_klt3 groups them): evaluations after the first at which a point that iterates is on new pixels while
    another one that iterates is not (mixed), at which one is (moved), and at which none is (kept)"""
    n = corner.shape[1]
    moved = np.zeros(iterating.shape, bool)
    moved[1:] = np.any(corner[1:] != corner[:-1], axis=2)
    mixed = reload = kept = 0
    for t in range(0, n, 3):
        it, mv = iterating[1:, t:t + 3], moved[1:, t:t + 3]
        live = it.any(1)
        mixed += int(((it & mv).any(1) & (it & ~mv).any(1)).sum())
        reload += int((live & (it & mv).any(1)).sum())
        kept += int((live & ~(it & mv).any(1)).sum())
    return mixed, reload, kept
