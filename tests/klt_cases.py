"""Named cases of the LK tracker for tests/test_klt_ref.py (CPU: the restatement tests/klt_ref.c against the oracle, and what the cases cover)
and tests/test_gpu_klt_ref.py (the device against the restatement, bit for bit).  A case is (pair, pts, init, prm): the name of a frame pair
of SIZES, reference points, initial guesses and the non-default fields of ygz_klt_params.  Every case is small: images of at most 352 x 352,
a few hundred points at most.

Points that reach one particular exit were found with the restatement (a seeded search over the 160 x 120 pair) and are written down here;
tests/test_klt_ref.py asserts from the restatement's taps that they still reach it.

  exits    every way a level can end, per kernel form (win 21: k_klt3; win 7 and 15: k_klt<false>)
  border   the reference window's corner at -win (kept) and -win - 1 (out), at w - 1 / w and h - 1 / h; guess the same limits for the
           searched window at the first evaluation.  Points are ip + half with integer ip, so that the floor is exact
  flat / checker   a textureless patch; a one-pixel pattern that pyrDown flattens exactly (coarse levels skipped, level 0 tracks)
  mineig   min_eig_threshold exactly the eigenvalue the restatement reports for point 1 (passes) and the next float above (fails)
  win / level / iter / eps / thr / noflow   one parameter varied over its edges, the other fields default, for both kernel forms
  shape / count   image sizes and point counts around the launch geometry (cells, points per pass)
  triple   win 21: every exit in each of the three positions of a wavefront's triple, beside two points that iterate
  walk_all   all 100 candidates of klt_window_case.walk(), the eight left-out ones included
  exact    pairs of so little contrast that every partial sum is an integer below 2^24: all orders and the oracle agree bit for bit
  filter   tracks ending exactly on the survivor rule's limits (ygz_hip_klt_track_filtered)"""
import functools

import numpy as np

import klt_ref
import klt_window_case as wc

CELL = 10                                      # the contexts' default cell size: cells = ceil(w / CELL) * ceil(h / CELL)
SHIFTS = wc.SHIFTS
KERNEL_WINS = (21, 7)                          # one window per kernel form (k_klt3, k_klt<false>)
WINS = (3, 4, 5, 7, 8, 11, 14, 15, 20, 21)     # the edges of the 7-pixel lane groups and of the row count
SIZES = {"small": (160, 120), "s96": (96, 64), "s37": (37, 29), "s37x33": (37, 33), "tall": (352, 352), "checker": (96, 64),
         "exact": (160, 120), "exact96": (96, 64)}
# ygz_hip_create refuses images below 32 pixels in either direction, so 37 x 29 (win 21: one level) exists on the CPU only -- the restatement
# against the oracle -- and 37 x 33, one level at win 21 as well, is the shape the device runs
DEVICE_MIN = 32


def on_device(pair):
    return min(SIZES[pair]) >= DEVICE_MIN


def cells(pair):
    w, h = SIZES[pair]
    return -(-w // CELL) * -(-h // CELL)


def _checker():
    """128 + (-1)^x g(y) + (-1)^y f(x): pyrDown's 1 4 6 4 1 taps weigh even and odd neighbours 8 : 8, so level 1 is exactly 128 everywhere,
    while level 0 has Scharr gradients 4 (-1)^y (f(x+1) - f(x-1)) and 4 (-1)^x (g(y+1) - g(y-1)) at whole-pixel positions"""
    rng = np.random.default_rng(41)
    w, h = SIZES["checker"]
    f, g = rng.integers(-50, 51, w), rng.integers(-50, 51, h)
    x, y = np.arange(w), np.arange(h)
    img = 128 + np.where(x % 2 == 0, 1, -1)[None, :] * g[:, None] + np.where(y % 2 == 0, 1, -1)[:, None] * f[None, :]
    assert img.min() >= 0 and img.max() <= 255
    img = np.ascontiguousarray(img, np.uint8)
    return [img, img.copy()]


def _low_contrast(imgs):
    return [np.ascontiguousarray(124 + (im >> 5), np.uint8) for im in imgs]


@functools.lru_cache(maxsize=None)
def pair(name):
    """the two frames (prev, next) of a named pair"""
    if name == "small":
        return wc._pair(wc.W, wc.H, 5, wc.FLAT)[0]
    if name == "s96":
        return wc._pair(96, 64, 7)[0]
    if name == "s37":
        return wc._pair(37, 29, 8)[0]
    if name == "s37x33":
        return wc._pair(37, 33, 9)[0]
    if name == "tall":
        return wc._pair(wc.TW, wc.TH, 6)[0]
    if name == "checker":
        return _checker()
    if name == "exact":
        return _low_contrast(pair("small"))
    if name == "exact96":
        return _low_contrast(pair("s96"))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def pyramids(name):
    imgs = pair(name)
    return klt_ref.pyramid(_oracle(), imgs[0]), klt_ref.pyramid(_oracle(), imgs[1])


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 2)


def _shifted(pts, first=0):
    pts = _f32(pts)
    return pts, (pts + SHIFTS[(np.arange(len(pts)) + first) % 4]).astype(np.float32)


def _rand(pair_name, seed, n, margin=4.0):
    w, h = SIZES[pair_name]
    rng = np.random.default_rng(seed)
    return _shifted(np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1))


def walk_candidates():
    """the 100 candidates klt_window_case.walk() draws before it leaves eight out"""
    rng = np.random.default_rng(29)
    pts = np.stack([rng.uniform(4, wc.W - 4, 80), rng.uniform(4, wc.H - 4, 80)], 1).astype(np.float32)
    more = np.stack([rng.uniform(4, wc.W - 4, 20), rng.uniform(4, wc.H - 4, 20)], 1).astype(np.float32)
    pts = np.concatenate([pts, more])
    return pts, (pts + SHIFTS[np.arange(len(pts)) % 4]).astype(np.float32)


# ---- points of the 160 x 120 pair that reach one exit at level 0 under the default parameters: (point, guess - point) ---------------------
NORMAL = [((55.25, 69.0), (3.5, -12.0)), ((130.25, 105.0), (0.0, 3.5))]                # converge / oscillate after several iterations
FLAT_POINT = (0.5 * (wc.FLAT[0] + wc.FLAT[2]), 0.5 * (wc.FLAT[1] + wc.FLAT[3]))
EXIT_POINTS = {
    21: {klt_ref.REF_OUT: ((-12.0, 60.0), (0.5, 0.0)), klt_ref.EIG_FAIL: (FLAT_POINT, (0.49, -0.49)),
         klt_ref.GUESS_OUT: ((157.75, 108.0), (5.0, 0.0)), klt_ref.CONVERGED: ((96.0, 99.75), (-6.0, 0.5)),
         klt_ref.OSCILLATION: ((43.75, 74.25), (0.5, 9.0)), klt_ref.MAX_ITER: ((35.25, 10.25), (0.5, -1.25)),
         klt_ref.ERR_OUT: ((23.5, 7.75), (0.5, 5.0))},
    7: {klt_ref.REF_OUT: ((-5.0, 60.0), (0.5, 0.0)), klt_ref.EIG_FAIL: (FLAT_POINT, (0.49, -0.49)),
        klt_ref.GUESS_OUT: ((86.0, 2.5), (-3.5, -1.25)), klt_ref.CONVERGED: ((43.75, 74.25), (0.5, 9.0)),
        klt_ref.OSCILLATION: ((130.25, 105.0), (0.0, 3.5)), klt_ref.MAX_ITER: ((96.0, 99.75), (-6.0, 0.5)),
        klt_ref.ERR_OUT: ((98.75, 9.5), (2.5, 5.0))},
}
# exits at a level above 0 (win 21, default parameters): the level is abandoned and the track goes on below
COARSE_POINTS = [((158.0, 13.0), (-12.0, -1.25)), ((154.5, 7.25), (15.0, -6.0)), ((145.0, 27.25), (0.0, -1.25)),      # guess window leaves at j >= 1
                 ((110.75, 1.25), (-6.0, -6.0)), ((1.25, 3.25), (0.5, -6.0)), ((107.25, -4.0), (-12.0, 15.0)),         # max_iter
                 ((75.75, 57.25), (9.0, 15.0)), ((76.5, 65.25), (9.0, 15.0)), ((80.25, 64.5), (-1.25, 9.0)),           # eigenvalue test (win 15, 7)
                 ((149.5, 126.25), (0.0, 9.0)), ((166.5, 92.0), (0.5, 0.5)), ((166.75, 2.0), (0.0, -12.0)),            # reference window (win 7)
                 ((-30.0, 60.0), (0.5, 0.0)), ((70.0, 141.0), (0.0, -0.5))]                                            # reference window (win 21: out at levels 1 and 0, inside at level 2)
# win 15, max_iter 1: one step from inside carries the error window out
ERR_OUT_15 = [((158.0, 13.0), (-12.0, -1.25)), ((57.0, 6.75), (0.5, 0.0)), ((139.0, 3.25), (-1.25, 3.5))]


def _pg(items):
    pts = _f32([p for p, _ in items])
    return pts, (pts + _f32([s for _, s in items])).astype(np.float32)


def _exits(win):
    return _pg([EXIT_POINTS[win][c] for c in klt_ref.EXITS] + NORMAL + COARSE_POINTS)


def _triples():
    """exit e at position k of its triple, the other two positions NORMAL: 7 exits x 3 positions x 3 points"""
    items = []
    for c in klt_ref.EXITS:
        for k in range(3):
            tri = list(NORMAL)
            tri.insert(k, EXIT_POINTS[21][c])
            items += tri
    return _pg(items)


def _border(win, guess):
    """window corners on the limits of the inside test, one per side and limit, then one ordinary point; the other coordinate mid-image"""
    w, h = SIZES["small"]
    half = (win - 1) * 0.5
    lim = [(-win, None), (-win - 1, None), (w - 1, None), (w, None), (None, -win), (None, -win - 1), (None, h - 1), (None, h)]
    edge = _f32([(50.0 + half if x is None else x + half, 70.0 + half if y is None else y + half) for x, y in lim] + [(50.0 + half, 70.0 + half)])
    if guess:                                  # ordinary reference points, the guesses on the limits
        pts = _f32([(20.0 + 5 * i, 95.0 + 2 * i) for i in range(len(edge))])      # clear of the textureless patch
        return pts, edge
    return _shifted(edge)


def _filter_edges():
    """max_iter 0 and one level: the track ends on its guess, bit for bit, so the survivor rule sees exactly these positions (borders 0 and 20)"""
    w, h = SIZES["small"]
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(-1e9)))
    g = []
    for b in (0.0, 20.0):
        g += [(b, 60.0), (below(b), 60.0), (w - b, 60.0), (below(w - b), 60.0), (80.0, b), (80.0, below(b)), (80.0, h - b), (80.0, below(h - b))]
    pts = _f32([(20.0 + 2 * i, 95.0 + i) for i in range(len(g))])                 # textured, clear of the borders
    return pts, _f32(g)


def _mineig(win, above):
    """three points of the small pair; the threshold is point 1's level-0 eigenvalue in the device's order, or the next float above it"""
    pts, init = _shifted([(96.0, 99.75), (43.75, 74.25), (55.25, 69.0)])
    pl, nl = pyramids("small")
    e = klt_ref.track(pl, nl, pts, init, klt_ref.device_order(win), win=win)["min_eig"][1, 0]
    thr = np.nextafter(np.float32(e), np.float32(np.inf)) if above else np.float32(e)
    return pts, init, dict(win=win, min_eig_threshold=float(thr))


def _build():
    C = {}
    small = wc.small()
    sp, si = _f32(small[3]), _f32(small[4])
    for win in KERNEL_WINS:
        t = "_w%d" % win
        C["exits" + t] = ("small",) + _exits(win) + (dict(win=win),)
        C["exits_thr0" + t] = ("small",) + _exits(win) + (dict(win=win, min_eig_threshold=0.0),)
        for ml in (0, 2):
            C["border_l%d%s" % (ml, t)] = ("small",) + _border(win, False) + (dict(win=win, max_level=ml),)
        C["guess_border" + t] = ("small",) + _border(win, True) + (dict(win=win, max_level=0),)
        C["mineig_at" + t] = ("small",) + _mineig(win, False)
        C["mineig_above" + t] = ("small",) + _mineig(win, True)
        for ml in (0, 1, 2, 4, 7):
            C["level%d%s" % (ml, t)] = ("small", sp, si, dict(win=win, max_level=ml))
        for mi in (-1, 0, 1, 2, 30, 100, 101):
            C["iter%d%s" % (mi, t)] = ("small", sp, si, dict(win=win, max_iter=mi))
        for k, eps in enumerate((-1.0, 0.0, 0.001, 0.03, 10.0, 11.0)):
            C["eps%d%s" % (k, t)] = ("small", sp, si, dict(win=win, eps=eps))
        for k, thr in enumerate((0.0, 1e-4, 1e3)):                                   # 1e3: above every patch's eigenvalue (<= (A11 + A22) / (2 win^2) <= 4080^2 / 2^20 < 16)
            C["thr%d%s" % (k, t)] = ("small", sp, si, dict(win=win, min_eig_threshold=thr))
        far = (sp + _f32([(1e4, -1e4)])).astype(np.float32)
        C["noflow" + t] = ("small", sp, far, dict(win=win, use_initial_flow=0))
        C["checker" + t] = ("checker",) + _pg([((40.0, 30.0), (0.0, 0.0)), ((60.0, 25.0), (0.25, 0.0)), ((30.0, 40.0), (2.0, 1.0)),
                                                ((70.5, 33.5), (0.0, 0.0))]) + (dict(win=win, max_level=1),)
        for name in ("s96", "s37", "s37x33", "tall"):
            C["shape_%s%s" % (name, t)] = (name,) + _rand(name, 60 + win, 10) + (dict(win=win),)
        ppp = wc.points_per_pass(cells("s96"))
        for n in (1, 2, 3, 4, 63, 64, 65, ppp - 1, ppp, ppp + 1, cells("s96"), cells("s96") + 1):
            C["count%d%s" % (n, t)] = ("s96",) + _rand("s96", 300 + n, n) + (dict(win=win),)
        for name in ("exact", "exact96"):
            C["%s%s" % (name, t)] = (name,) + _rand(name, 80 + win, 12, margin=8.0) + (dict(win=win, min_eig_threshold=0.0),)
    for win in WINS:
        C["win%d" % win] = ("small", sp, si, dict(win=win))
    C["win3_level7"] = ("small", sp, si, dict(win=3, max_level=7))
    C["tall_level7_w7"] = ("tall",) + _rand("tall", 71, 10) + (dict(win=7, max_level=7),)
    C["exits_w15"] = ("small",) + _exits(7) + (dict(win=15),)
    C["err_out_w15"] = ("small",) + _pg(ERR_OUT_15 + NORMAL) + (dict(win=15, max_iter=1),)
    C["exact_w15"] = ("exact",) + _rand("exact", 95, 12, margin=8.0) + (dict(win=15, min_eig_threshold=0.0),)
    C["small"] = ("small", sp, si, {})
    C["walk"] = ("small",) + tuple(_f32(a) for a in wc.walk()) + ({},)
    C["walk_all"] = ("small",) + walk_candidates() + ({},)
    C["triple"] = ("small",) + _triples() + ({},)
    C["filter_w21"] = ("small",) + _filter_edges() + (dict(max_iter=0, max_level=0),)
    C["filter_w7"] = ("small",) + _filter_edges() + (dict(win=7, max_iter=0, max_level=0),)
    for t in (1, 2, 4):
        timgs, tpts, tinit = wc.tall()
        C["tall%d" % t] = ("tall", _f32(tpts[:t]), _f32(tinit[:t]), {})
    return C


@functools.lru_cache(maxsize=None)
def cases():
    return _build()


def names(pair_name=None):
    return [k for k, v in cases().items() if pair_name is None or v[0] == pair_name]


def get(name):
    """(pair, pts, init, prm)"""
    return cases()[name]


def is_exact(name):
    return get(name)[0].startswith("exact")


@functools.lru_cache(maxsize=None)
def reference(name, order=None):
    """the restatement on a case, in the device's order unless another is given (computed once, shared, never written to)"""
    pr, pts, init, prm = get(name)
    pl, nl = pyramids(pr)
    win = prm.get("win", 21)
    r = klt_ref.track(pl, nl, pts, init, klt_ref.device_order(win) if order is None else order, **prm)
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r
