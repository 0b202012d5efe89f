"""Crafted pictures that put one corner ON each limit of the extractor (ygz_slam_amd/csrc/detect.hip: k_fast_select, k_compact, k_describe;
DESIGN.md section 38, steps 1-10).  tests/test_extract_cases.py holds them to the oracle and to a numpy witness on the CPU,
tests/test_gpu_extract_limits.py runs them on the device.  Pure numpy, all-integer: no random number is drawn, no transcendental is called,
so the pictures are the same bytes on every machine.

A case is Case(row, name, picture, params, occupied, probes, expected):
  picture   level 0, uint8 [h, w]; the lower levels are the pyramid of it
  params    levels, fast_threshold, cell_size, nms_tie_suppress, debug_maps: the arguments of the context
  occupied  None or the uint8 mask of the grid cells
  probes    [(level, x, y)]: the pixels whose stored FAST score (score + 1, 0 = no corner) and NMS flag are literals of the case
  expected  keypoints [(px, py, level, score bits)] in output order (an empty list is the literal absence), score [byte per probe],
            nms [flag per probe], all from LITERALS below
The pictures are built from two designed stamps on a flat background of BG:
  ring stamp  a centre pixel p and its sixteen ring pixels p + diff[k], k in the order of RING: which pixels are brighter than p + t or
              darker than p - t, the longest arc and the score (the largest t for which the arc still holds) are read off the sixteen numbers;
              the builders write the stored byte next to the stamp and the module asserts it against LITERALS.  A dot is the stamp whose
              ring is the background: p = BG + d, d > t, is a corner of FAST score d - 1 and of Shi-Tomasi score exactly d * d / 64
              (dXX = dYY = 2 d^2 / 128, dXY = 0, discriminant 0), and with d <= 2 t nothing else in the picture is a corner.
  bump        amp * (1 - r^2 / R^2)^2 with R = rr * 2^L, in integers: smooth enough that no level below L has a corner at the case's
              threshold, and after L halvings one corner at exactly (cx / 2^L, cy / 2^L).  A level above 0 cannot be painted directly (the
              pyramid is built on the device), so corners of levels 1-3 are bumps and their scores are the oracle's, recorded in LITERALS.

Sizes.  UNIT 208 x 136 (w % 4 == 0: level 0 has the interior tile bx = 1, by = 1..2 and edge tiles elsewhere; levels 1, 2 are 104 x 68 and
52 x 34, edge tiles only).  TWIN 206 x 135: every level on the byte staging path, levels of odd width (103, 52).  A level-L corner is kept only
for 20 * 2^L <= x (step 4), its Shi-Tomasi window fits only for x <= w_L - 6 (step 7), so level L needs w_L >= 20 * 2^L + window + 5 for a
window of `window` positions; square(L, window) rounds w_L up to a multiple of 4 (every level on the dword path) and returns w_L * 2^L:
LEVEL2 = square(2, 24) = 448 (level-2 positions 80..108: the cell-64 boundary px 384 with room on both sides), LEVEL3 = square(3, 8) = 1408.
At UNIT no level-2 corner can be kept (52 < 80), and levels >= 4 cannot yield a feature below 5121 pixels: they are covered by the
configuration sweep alone.

No NaN row.  A NaN Shi-Tomasi score cannot occur: the three gradient sums are integers below 2^22 scaled by 2^-7, tr = dXX + dYY is exact in
float, and fl(tr^2) >= 4 fl(dXX dYY) >= 4 fl(fl(dXX dYY) - fl(dXY^2)) because rounding is monotone (dXX dYY <= tr^2 / 4, and subtracting a
non-negative number and rounding cannot exceed the rounded minuend), so the discriminant is never negative.  A search over 8e7 admissible
triples on the CPU found none.  The kernel's NaN key stays as it is; do not go looking for a picture."""
import collections

import numpy as np

BG = 100
UNIT, TWIN = (208, 136), (206, 135)
# ring position k -> (dx, dy): FAST's Bresenham circle of radius 3
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
ROWS = ("FAST test", "FAST score", "FAST border", "NMS", "InFrame", "cell index", "occupied", "cell winner", "Shi-Tomasi window", "output",
        "level 3")

Case = collections.namedtuple("Case", "row name picture params occupied probes expected")


def square(L, window):
    wl = 20 * 2 ** L + window + 5
    return (-(-wl // 4) * 4) << L


LEVEL2 = (square(2, 24), square(2, 24))
LEVEL3 = (square(3, 8), square(3, 8))
assert LEVEL2 == (448, 448) and LEVEL3 == (1408, 1408)


def level_size(size, L):
    w, h = size
    for _ in range(L):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def grid(size, cell):
    return -(-size[0] // cell), -(-size[1] // cell)


def cell_of(size, cell, L, x, y):
    """step 5 for a level coordinate"""
    return ((y << L) // cell) * grid(size, cell)[0] + (x << L) // cell


def flat(size, bg=BG):
    return np.full((size[1], size[0]), bg, np.uint8)


def ring_stamp(img, x, y, p, diffs):
    assert len(diffs) == 16 and all(0 <= p + d <= 255 for d in diffs)
    img[y, x] = p
    for (dx, dy), d in zip(RING, diffs):
        img[y + dy, x + dx] = p + d


def dot(img, x, y, d):
    img[y, x] = BG + d


def bump(img, X, Y, L, amp=30, rr=3):
    """adds the bump of level L centred on level-L pixel (X, Y)"""
    h, w = img.shape
    cx, cy, R = X << L, Y << L, rr << L
    ys, xs = np.mgrid[max(0, cy - R):min(h, cy + R + 1), max(0, cx - R):min(w, cx + R + 1)]
    q = np.maximum(R * R - (xs - cx) ** 2 - (ys - cy) ** 2, 0).astype(np.int64)
    img[ys, xs] = (img[ys, xs].astype(np.int64) + (amp * q * q + R ** 4 // 2) // R ** 4).astype(np.uint8)


def shi_dot(d):
    """score bits of an isolated dot"""
    return int(np.float32(d * d / 64.0).view(np.uint32))


def prm(levels=1, thr=15, cell=10, tie=0, maps=True):
    return dict(levels=levels, fast_threshold=thr, cell_size=cell, nms_tie_suppress=tie, debug_maps=maps)


_cases = []


def case(row, name, img, params, probes=(), designed=None, occupied=None, keypoints=None):
    """designed: the stored bytes the builder derived by hand for the probes (None: the oracle's); keypoints: a hand-derived literal list"""
    name = "%s/%s" % (row, name)
    assert name not in {c.name for c in _cases}, name
    lit = LITERALS.get(name.replace("debug_maps off", "debug_maps on"))      # the keypoints must not depend on debug_maps: one literal for both
    if lit is None and keypoints is not None and not probes:
        lit = dict(keypoints=[tuple(k) for k in keypoints], score=[], nms=[])  # dots only: the whole literal is derived where the case is built
    if lit is not None:
        assert len(lit["score"]) == len(lit["nms"]) == len(probes), name
        if designed is not None:
            assert [b for b in designed] == [s for s in lit["score"]], (name, designed, lit["score"])
        if keypoints is not None:
            assert [tuple(k) for k in keypoints] == [tuple(k) for k in lit["keypoints"]], (name, keypoints, lit["keypoints"])
    _cases.append(Case(row, name, img, params, occupied, list(probes), lit))


# ---- FAST test (step 1) ------------------------------------------------------------------------------------------------------------------------
def _fast_test():
    """per threshold one picture of stamps on a 12-pixel lattice; each stamp's centre is a probe.  s = t + 1 is the first value that counts"""
    for t in (0, 1, 15, 40, 254):
        s = t + 1
        wrap = [s if (k >= 11 or k <= 4) else 0 for k in range(16)]
        stamps = [("arc 10 one step inside", [s] * 10 + [0] * 6, s), ("arc 10 on p+t", [t] * 10 + [0] * 6, 0),
                  ("arc 9", [s] * 9 + [t] + [0] * 6, 0), ("arc wraps 15->0", wrap, s), ("arc 10, the rest on p+t", [s] * 10 + [t] * 6, s),
                  ("arc 11 with a gap", [s] * 5 + [t] + [s] * 5 + [0] * 5, 0)]
        img, probes, designed = flat(UNIT), [], []
        for sign, p in ((1, 0 if t == 254 else BG), (-1, 255 if t == 254 else BG)):
            for i, (_, diffs, byte) in enumerate(stamps):
                x, y = 30 + 12 * i, 40 if sign > 0 else 60
                ring_stamp(img, x, y, p, [sign * d for d in diffs])
                probes.append((0, x, y)); designed.append(byte)
        if t != 254:                                          # five brighter and five darker must not combine
            ring_stamp(img, 30, 80, BG, [s] * 5 + [-s] * 5 + [0] * 6)
            probes.append((0, 30, 80)); designed.append(0)
            ring_stamp(img, 42, 80, BG, [s] * 9 + [-s] * 7)
            probes.append((0, 42, 80)); designed.append(0)
        case("FAST test", "threshold %d: on, inside and outside p+-t, arcs of 9 and 10" % t, img, prm(thr=t, cell=64), probes, designed)


# ---- FAST score (step 2) -----------------------------------------------------------------------------------------------------------------------
def _fast_score():
    stamps = [(BG, [18] * 3 + [25] * 10 + [0] * 3, 25),                                                   # the second arc is the best one
              (150, [-v for v in (17, 40, 35, 50, 22, 60, 33, 45, 28, 70, 26, 19, 0, 0, 0, 0)], 22),     # arcs from 0: 17, from 1: 22, from 2: 19
              (0, [255] * 16, 255), (255, [-255] * 16, 255),                                              # score 254, stored 255
              (BG, [16] * 12 + [0] * 4, 16),                                                              # score == threshold, stored thr + 1
              (60, [20 + k for k in range(16)], 26),                                                      # a ramp: the arc 6..15
              (BG, [-v for v in [50] * 6 + [0] * 6 + [50] * 4], 50),                                      # the best arc wraps
              (BG, [15] * 16, 0),                                                                         # the whole ring on p + t
              (BG, [40] * 9 + [16] + [0] * 6, 16), (BG, [-40] * 9 + [-15] + [0] * 6, 0)]
    img, probes = flat(UNIT), []
    for i, (p, diffs, _) in enumerate(stamps):
        ring_stamp(img, 30 + 14 * i, 50, p, diffs)
        probes.append((0, 30 + 14 * i, 50))
    case("FAST score", "the largest t of each stamp at threshold 15", img, prm(cell=64), probes, [s[2] for s in stamps])
    img, probes = flat(UNIT), []
    for i, (p, diffs, _) in enumerate(stamps):
        ring_stamp(img, 30 + 14 * i, 50, p, diffs)
        probes.append((0, 30 + 14 * i, 50))
    # at threshold 40 the scores stay, the stamps below it leave
    case("FAST score", "the same stamps at threshold 40", img, prm(thr=40, cell=64), probes, [s[2] if s[2] > 40 else 0 for s in stamps])


# ---- FAST border (step 1's domain) ---------------------------------------------------------------------------------------------------------------
def _fast_border():
    w, h = TWIN
    img = flat(TWIN)
    spots = [(3, 12, 25), (2, 24, 0), (w - 4, 12, 25), (w - 3, 24, 0), (30, 3, 25), (42, 2, 0), (30, h - 4, 25), (42, h - 3, 0)]
    for x, y, _ in spots:
        dot(img, x, y, 25)
    case("FAST border", "level 0 of 206 x 135: x = 3 | 2, w-4 | w-3, the same for y", img, prm(levels=1), [(0, x, y) for x, y, _ in spots],
         [b for _, _, b in spots])
    w1, h1 = level_size(TWIN, 1)
    img = flat(TWIN)
    spots = [(3, 20), (2, 34), (w1 - 4, 20), (w1 - 3, 34), (30, 3), (44, 2), (30, h1 - 4), (44, h1 - 3)]
    for X, Y in spots:
        bump(img, X, Y, 1, 40, 4)
    case("FAST border", "level 1 (103 x 68): x = 3 | 2, w-4 | w-3, the same for y", img, prm(levels=2), [(1, X, Y) for X, Y in spots])
    w2, h2 = level_size(TWIN, 2)
    for name, spots in (("x = 3 | 2, w-4 | w-3", [(3, 9), (2, 24), (w2 - 4, 9), (w2 - 3, 24)]),
                        ("y = 3 | 2, h-4 | h-3", [(12, 3), (36, 2), (12, h2 - 4), (36, h2 - 3)])):
        img = flat(TWIN)
        for X, Y in spots:
            bump(img, X, Y, 2, 40, 4)
        case("FAST border", "level 2 (52 x 34): " + name, img, prm(levels=3), [(2, X, Y) for X, Y in spots])


# ---- NMS (step 3) ------------------------------------------------------------------------------------------------------------------------------
def _nms():
    pairs = [((40, 50), (41, 50)), ((60, 50), (60, 51)), ((80, 50), (81, 51)), ((101, 50), (100, 51)),       # -, |, \, /
             ((63, 70), (64, 70)), ((90, 31), (90, 32)), ((63, 31), (64, 32)), ((128, 63), (127, 64))]     # across the tile seams and a tile corner
    for tie in (0, 1):
        img, probes, designed = flat(UNIT), [], []
        for a, b in pairs:
            dot(img, a[0], a[1], 25); dot(img, b[0], b[1], 25)
            probes += [(0,) + a, (0,) + b]; designed += [25, 25]
        for (x, y), (x2, y2) in (((120, 50), (121, 50)), ((140, 50), (141, 51)), ((64, 90), (63, 91))):      # a neighbour stronger by exactly 1
            dot(img, x, y, 25); dot(img, x2, y2, 26)
            probes += [(0, x, y), (0, x2, y2)]; designed += [25, 26]
        case("NMS", "equal 8-neighbours and a neighbour stronger by 1, nms_tie_suppress = %d" % tie, img, prm(cell=1, tie=tie), probes, designed)


# ---- InFrame(20, L) (step 4) -------------------------------------------------------------------------------------------------------------------
def _inframe():
    w, h = UNIT
    for maps in (True, False):
        tag = ", debug_maps %s" % ("on" if maps else "off")
        img = flat(UNIT)
        kept = [(20, 50), (100, 20), (w - 21, 70), (70, h - 21)]
        for x, y in kept + [(19, 90), (130, 19), (w - 20, 30), (150, h - 20)]:
            dot(img, x, y, 25)
        kps = sorted(kept, key=lambda p: cell_of(UNIT, 10, 0, *p))
        case("InFrame", "level 0: x = 20 | 19, cols-21 | cols-20, the same for y" + tag, img, prm(levels=1, maps=maps),
             keypoints=[(float(x), float(y), 0, shi_dot(25)) for x, y in kps])
        w1, h1 = level_size(UNIT, 1)
        for name, spots in (("on the limit: x = 40, y = 40, x = w1-4", [(40, 60), (70, 40), (w1 - 4, 50)]),
                            ("one step outside: x = 39, y = 39", [(39, 60), (70, 39)])):
            img = flat(UNIT)
            for X, Y in spots:
                bump(img, X, Y, 1)
            case("InFrame", "level 1: " + name + tag, img, prm(levels=2, maps=maps))
        w2, h2 = level_size(LEVEL2, 2)
        for name, spots in (("on the limit: x = 80, y = 80, x = w2-4", [(80, 100), (100, 80), (w2 - 4, 100)]),
                            ("one step outside: x = 79, y = 79", [(79, 100), (100, 79)])):
            img = flat(LEVEL2)
            for X, Y in spots:
                bump(img, X, Y, 2)
            case("InFrame", "level 2: " + name + tag, img, prm(levels=3, maps=maps))


# ---- cell index (step 5) -----------------------------------------------------------------------------------------------------------------------
def _boundaries(cell, L, lo, hi):
    """the level-L coordinates (a, a + 1) in [lo, hi], from the top, with (v << L) // cell on either side of a cell boundary: the last of
    one cell and the first of the next (where 2^L does not divide the boundary it falls between two level pixels)"""
    return [(a, a + 1) for a in range(hi - 1, lo - 1, -1) if (a << L) // cell != ((a + 1) << L) // cell]


def _cell_index():
    """four corners per picture, two across a boundary in x (on the first and the last admissible row) and two across one in y (on the last
    and the first admissible column).  Every grid cell is flagged as occupied except the four cells the corners belong to: a corner given
    any other cell index disappears, and two given the same one merge.  Level 1 is taken at the larger size: at 208 x 136 its admissible
    rows 40..62 hold no boundary of cell 64"""
    for L, size in ((0, UNIT), (1, LEVEL2), (2, LEVEL2)):
        wl, hl = level_size(size, L)
        lo, gap = 20 << L, 8 if L else 9
        x_hi, y_hi = (wl - 6, hl - 6) if L else (size[0] - 21, size[1] - 21)
        for cell in (1, 3, 4, 7, 10, 16, 64):
            (xa, xb) = _boundaries(cell, L, lo + gap, x_hi - gap - 1)[0]
            (ya, yb) = _boundaries(cell, L, lo + gap, y_hi - gap - 1)[0]
            spots = [(xa, lo), (xb, y_hi), (x_hi, ya), (lo, yb)]
            assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) >= gap for i, p in enumerate(spots) for q in spots[:i]), (L, cell, spots)
            img = flat(size)
            for X, Y in spots:
                dot(img, X, Y, 25) if L == 0 else bump(img, X, Y, L)
            cols, rows = grid(size, cell)
            occ = np.ones(cols * rows, np.uint8)
            ks = [cell_of(size, cell, L, X, Y) for X, Y in spots]
            assert len(set(ks)) == len(spots), (L, cell, spots, ks)
            occ[ks] = 0
            kps = None
            if L == 0:
                kps = [(float(x), float(y), 0, shi_dot(25)) for _, (x, y) in sorted(zip(ks, spots))]
            case("cell index", "cell %d, level %d: x = %d | %d, y = %d | %d" % (cell, L, xa, xb, ya, yb), img,
                 prm(levels=L + 1, cell=cell, maps=False), occupied=occ, keypoints=kps)


# ---- occupied (step 6) -------------------------------------------------------------------------------------------------------------------------
def _occupied():
    """a dot (level 0), and bumps of levels 1 and 2 where the size has them, each alone in its cell.  "flagged": exactly their cells are
    occupied and nothing is left; "neighbours flagged": the eight cells around each are occupied instead and every corner is kept"""
    for cell, size, levels in ((10, UNIT, 3), (3, UNIT, 3), (4, LEVEL2, 3), (3, LEVEL2, 3)):
        img = flat(size)
        if size == UNIT:
            spots = [(0, 50, 50), (0, 150, 60), (1, 45, 52), (1, 80, 45)]
        else:
            spots = [(0, 50, 50), (0, 300, 90), (1, 60, 150), (1, 190, 100), (2, 85, 90), (2, 100, 104)]
        for L, X, Y in spots:
            dot(img, X, Y, 25) if L == 0 else bump(img, X, Y, L)
        cols, rows = grid(size, cell)
        ks = [cell_of(size, cell, L, X, Y) for L, X, Y in spots]
        on = np.zeros(cols * rows, np.uint8)
        on[ks] = 1
        around = np.zeros(cols * rows, np.uint8)
        for k in ks:
            for dk in (-cols - 1, -cols, -cols + 1, -1, 1, cols - 1, cols, cols + 1):
                around[k + dk] = 1
        assert not around[ks].any()
        tag = "cell %d, %d x %d" % ((cell,) + size)
        case("occupied", tag + ": the corners' cells flagged", img, prm(levels=levels, cell=cell, maps=False), occupied=on, keypoints=[])
        case("occupied", tag + ": the neighbours flagged", img, prm(levels=levels, cell=cell, maps=False), occupied=around)
        case("occupied", tag + ": no mask", img, prm(levels=levels, cell=cell, maps=False))


# ---- cell winner (step 8) ----------------------------------------------------------------------------------------------------------------------
def _winner():
    def dots(name, spots, win):
        img = flat(UNIT)
        for x, y, d in spots:
            dot(img, x, y, d)
        case("cell winner", name, img, prm(levels=1), keypoints=[(float(x), float(y), 0, shi_dot(d)) for x, y, d in win])
    # one cell (x 30..39, y 30..39), candidates 9 pixels apart: no dot inside another's Shi-Tomasi window
    dots("two in a cell: the stronger is visited second", [(30, 30, 20), (39, 39, 28)], [(39, 39, 28)])
    dots("two in a cell: the stronger is visited first", [(30, 30, 28), (39, 39, 20)], [(30, 30, 28)])
    dots("three in a cell: the strongest is visited second", [(30, 30, 20), (39, 30, 28), (30, 39, 24)], [(39, 30, 28)])
    dots("three in a cell: stronger by one step of d", [(30, 30, 27), (39, 30, 26), (30, 39, 28)], [(30, 39, 28)])
    dots("tie: (x small, y large) against (x large, y small) goes to the smaller y", [(30, 39, 25), (39, 30, 25)], [(39, 30, 25)])
    dots("tie in one row goes to the smaller x", [(30, 35, 25), (39, 35, 25)], [(30, 35, 25)])
    dots("tie of three: the first in raster order", [(39, 39, 25), (30, 39, 25), (35, 30, 25)], [(35, 30, 25)])
    # across levels.  cell 16, cell (6, 5): x 96..111, y 80..95
    img = flat(UNIT)
    dot(img, 98, 82, 16)
    bump(img, 54, 45, 1)
    case("cell winner", "level 1 strictly greater than level 0 replaces it", img, prm(levels=2, cell=16))
    # the exact tie across levels: the Shi-Tomasi window of both corners leaves the level (step 7), both score the literal 0.0 and fall
    # into one cell of 64; level 1 is visited first
    w1, _ = level_size(LEVEL2, 1)
    w2, _ = level_size(LEVEL2, 2)
    for name, l1, l2 in (("both levels", True, True), ("level 2 alone", False, True), ("level 1 alone", True, False)):
        img = flat(LEVEL2)
        if l1:
            bump(img, w1 - 5, 165, 1)
        if l2:
            bump(img, w2 - 5, 92, 2)
        case("cell winner", "tie at 0.0 across levels 1 and 2 in one cell: " + name, img, prm(levels=3, cell=64))
    # a cell whose only candidate scores 0.0 is still a keypoint
    img = flat(UNIT)
    bump(img, level_size(UNIT, 1)[0] - 5, 50, 1)
    case("cell winner", "the only candidate of a cell scores 0.0", img, prm(levels=2))


# ---- Shi-Tomasi window (step 7) ----------------------------------------------------------------------------------------------------------------
def _shi_window():
    w1, h1 = level_size(UNIT, 1)
    for name, spots in (("level 1: the window just fits, x = w1-6, y = h1-6", [(w1 - 6, 45), (60, h1 - 6)]),
                        ("level 1: one pixel further out, x = w1-5, y = h1-5", [(w1 - 5, 45), (60, h1 - 5)])):
        img = flat(UNIT)
        for X, Y in spots:
            bump(img, X, Y, 1)
        case("Shi-Tomasi window", name, img, prm(levels=2))
    w2, h2 = level_size(LEVEL2, 2)
    for name, spots in (("level 2: the window just fits, x = w2-6, y = h2-6", [(w2 - 6, 85), (85, h2 - 6)]),
                        ("level 2: one pixel further out, x = w2-5, y = h2-5", [(w2 - 5, 85), (85, h2 - 5)])):
        img = flat(LEVEL2)
        for X, Y in spots:
            bump(img, X, Y, 2)
        case("Shi-Tomasi window", name, img, prm(levels=3))


# ---- output (step 9) ---------------------------------------------------------------------------------------------------------------------------
def _output():
    """dots and level-1 bumps painted in an order that is not the cell order.  cells = 28288 at cell 1, 7072 at cell 2, 294 at cell 10 and
    12 at cell 64: k_compact runs with 28, 7 and 1 cells per thread, and with fewer cells than threads"""
    img = flat(UNIT)
    spots = [(0, 170, 100, 22), (0, 30, 95, 27), (0, 99, 21, 18), (0, 100, 60, 30), (0, 21, 22, 25), (0, 187, 115, 16), (0, 64, 64, 29), (0, 63, 33, 21),
             (1, 80, 55, 0), (1, 45, 44, 0), (1, 99, 62, 0)]
    for L, X, Y, d in spots:
        dot(img, X, Y, d) if L == 0 else bump(img, X, Y, L)
    for cell in (1, 2, 10, 64):
        assert grid(UNIT, cell)[0] * grid(UNIT, cell)[1] == {1: 28288, 2: 7072, 10: 294, 64: 12}[cell]
        case("output", "cell order, px = x * 2^L, the count: cell %d" % cell, img, prm(levels=2, cell=cell, maps=False))
    case("output", "no corner at all", flat(UNIT), prm(levels=3, maps=False), keypoints=[])


# ---- level 3 -----------------------------------------------------------------------------------------------------------------------------------
def _level3():
    w3, _ = level_size(LEVEL3, 3)
    img = flat(LEVEL3)
    for X, Y in ((160, 163), (168, 159), (w3 - 5, w3 - 5), (159, w3 - 4)):        # on the limit, y outside, window outside (0.0), x outside
        bump(img, X, Y, 3)
    dot(img, 700, 700, 25)
    case("level 3", "x = 160 | 159, y = 159, the window at w3-5", img, prm(levels=4, maps=False))


# ---- embedding ---------------------------------------------------------------------------------------------------------------------------------
FILLER_DOTS = ((50, 50, 25), (90, 70, 20))


def filler(size):
    """the picture of the other slots when a case is run among 17: two dots"""
    img = flat(size)
    for x, y, d in FILLER_DOTS:
        dot(img, x, y, d)
    return img


def filler_keypoints(params):
    """the filler's literals under a case's parameters: a dot of d > threshold is a corner, the two never share a cell or a window"""
    return [(float(x), float(y), 0, shi_dot(d)) for x, y, d in FILLER_DOTS if d > params["fast_threshold"]]


def holds(c, keypoints, score_maps=None, nms_maps=None):
    """the departures of an extractor's outputs from the literals of case c: keypoints [(px, py, level, score bits)] in output order, and,
    where the case has probes, the stored-score and NMS maps per level"""
    bad = []
    want = [tuple(k) for k in c.expected["keypoints"]]
    got = [(float(a), float(b), int(l), int(s)) for a, b, l, s in keypoints]
    if got != want:
        bad.append(("keypoints", got, want))
    for i, (L, x, y) in enumerate(c.probes):
        if score_maps is not None and int(score_maps[L][y, x]) != c.expected["score"][i]:
            bad.append(("score", (L, x, y), int(score_maps[L][y, x]), c.expected["score"][i]))
        if nms_maps is not None and int(nms_maps[L][y, x]) != c.expected["nms"][i]:
            bad.append(("nms", (L, x, y), int(nms_maps[L][y, x]), c.expected["nms"][i]))
    return bad


# ---- the literals --------------------------------------------------------------------------------------------------------------------------------
# name -> keypoints [(px, py, level, score bits)], score / nms per probe.  Written once from the oracle's outputs and then frozen:
# tests/test_extract_cases.py asserts that the oracle and the witness both still give them, and the builders above assert every value they
# derived by hand (`designed`, `keypoints`) against this table when the module is imported.
D25 = 0x411C4000                # 25 * 25 / 64 = 9.765625, the dot of d = 25
B1, B2 = 0x41F51000, 0x41EFF000  # 30.6328125 and 29.9921875: the bump of amp 30, rr 3 seen at level 1 and at levels 2 and 3, its window inside the level
_OCC_UNIT = [(50.0, 50.0, 0, D25), (150.0, 60.0, 0, D25), (160.0, 90.0, 1, B1), (90.0, 104.0, 1, B1)]
_OCC_LEVEL2 = [(50.0, 50.0, 0, D25), (300.0, 90.0, 0, D25), (380.0, 200.0, 1, B1), (120.0, 300.0, 1, B1), (340.0, 360.0, 2, B2), (400.0, 416.0, 2, B2)]
_OUT_FINE = [(99.0, 21.0, 0, 0x40A20000), (21.0, 22.0, 0, D25), (63.0, 33.0, 0, 0x40DC8000), (100.0, 60.0, 0, 0x41610000), (64.0, 64.0, 0, 0x41524000),
             (90.0, 88.0, 1, B1), (30.0, 95.0, 0, 0x41364000), (170.0, 100.0, 0, 0x40F20000), (160.0, 110.0, 1, B1), (187.0, 115.0, 0, 0x40800000),
             (198.0, 124.0, 1, 0)]
LITERALS = {
    "FAST test/threshold 0: on, inside and outside p+-t, arcs of 9 and 10": dict(
        keypoints=[(33.0, 40.0, 0, 0x3E000000), (81.0, 40.0, 0, 0x3E000000), (44.0, 82.0, 0, 0x3E180000)],
        score=[1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0], nms=[1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0]),
    "FAST test/threshold 1: on, inside and outside p+-t, arcs of 9 and 10": dict(
        keypoints=[(33.0, 40.0, 0, 0x3F000000), (78.0, 40.0, 0, 0x3F0698CD), (44.0, 82.0, 0, 0x3F180000)],
        score=[2, 0, 0, 2, 2, 0, 2, 0, 0, 2, 2, 0, 0, 0], nms=[1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0]),
    "FAST test/threshold 15: on, inside and outside p+-t, arcs of 9 and 10": dict(
        keypoints=[(33.0, 40.0, 0, 0x42000000), (78.0, 40.0, 0, 0x423CFD96), (44.0, 82.0, 0, 0x42180000)],
        score=[16, 0, 0, 16, 16, 0, 16, 0, 0, 16, 16, 0, 0, 0], nms=[1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0]),
    "FAST test/threshold 40: on, inside and outside p+-t, arcs of 9 and 10": dict(
        keypoints=[(33.0, 40.0, 0, 0x43522002), (78.0, 40.0, 0, 0x43A08DCC), (44.0, 82.0, 0, 0x43798600)],
        score=[41, 0, 0, 41, 41, 0, 41, 0, 0, 41, 41, 0, 0, 0], nms=[1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0]),
    "FAST test/threshold 254: on, inside and outside p+-t, arcs of 9 and 10": dict(
        keypoints=[(30.0, 40.0, 0, 0x455FF204), (78.0, 40.0, 0, 0x4596A842)],
        score=[255, 0, 0, 255, 255, 0, 255, 0, 0, 255, 255, 0], nms=[1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0]),
    "FAST score/the largest t of each stamp at threshold 15": dict(
        keypoints=[(58.0, 50.0, 0, 0x45978510), (72.0, 50.0, 0, 0x45118840), (142.0, 50.0, 0, 0x43330000)],
        score=[25, 22, 255, 255, 16, 26, 50, 0, 16, 0], nms=[1, 1, 1, 1, 1, 1, 1, 0, 1, 0]),
    "FAST score/the same stamps at threshold 40": dict(
        keypoints=[(58.0, 50.0, 0, 0x45978510), (72.0, 50.0, 0, 0x45118840)],
        score=[0, 0, 255, 255, 0, 0, 50, 0, 0, 0], nms=[0, 0, 1, 1, 0, 0, 1, 0, 0, 0]),
    "FAST border/level 0 of 206 x 135: x = 3 | 2, w-4 | w-3, the same for y": dict(
        keypoints=[], score=[25, 0, 25, 0, 25, 0, 25, 0], nms=[1, 0, 1, 0, 1, 0, 1, 0]),
    "FAST border/level 1 (103 x 68): x = 3 | 2, w-4 | w-3, the same for y": dict(
        keypoints=[(88.0, 128.0, 1, 0)], score=[28, 0, 28, 0, 28, 0, 28, 0], nms=[1, 0, 1, 0, 1, 0, 1, 0]),
    "FAST border/level 2 (52 x 34): x = 3 | 2, w-4 | w-3": dict(keypoints=[], score=[27, 0, 27, 0], nms=[1, 0, 1, 0]),
    "FAST border/level 2 (52 x 34): y = 3 | 2, h-4 | h-3": dict(keypoints=[], score=[27, 0, 27, 0], nms=[1, 0, 1, 0]),
    "NMS/equal 8-neighbours and a neighbour stronger by 1, nms_tie_suppress = 0": dict(
        keypoints=[(63.0, 31.0, 0, D25), (90.0, 31.0, 0, 0x419C4000), (64.0, 32.0, 0, D25), (90.0, 32.0, 0, 0x419C4000), (40.0, 50.0, 0, 0x419C4000),
                   (41.0, 50.0, 0, 0x419C4000), (60.0, 50.0, 0, 0x419C4000), (80.0, 50.0, 0, D25), (101.0, 50.0, 0, D25), (121.0, 50.0, 0, 0x41A2A000),
                   (60.0, 51.0, 0, 0x419C4000), (81.0, 51.0, 0, D25), (100.0, 51.0, 0, D25), (141.0, 51.0, 0, 0x4122C000), (128.0, 63.0, 0, D25),
                   (127.0, 64.0, 0, D25), (63.0, 70.0, 0, 0x419C4000), (64.0, 70.0, 0, 0x419C4000), (63.0, 91.0, 0, 0x4122C000)],
        score=[25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 26, 25, 26, 25, 26],
        nms=[1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 0, 1]),
    "NMS/equal 8-neighbours and a neighbour stronger by 1, nms_tie_suppress = 1": dict(
        keypoints=[(121.0, 50.0, 0, 0x41A2A000), (141.0, 51.0, 0, 0x4122C000), (63.0, 91.0, 0, 0x4122C000)],
        score=[25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 25, 26, 25, 26, 25, 26],
        nms=[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1]),
    "InFrame/level 1: on the limit: x = 40, y = 40, x = w1-4, debug_maps on": dict(
        keypoints=[(140.0, 80.0, 1, B1), (200.0, 100.0, 1, 0), (80.0, 120.0, 1, B1)], score=[], nms=[]),
    "InFrame/level 1: one step outside: x = 39, y = 39, debug_maps on": dict(keypoints=[], score=[], nms=[]),
    "InFrame/level 2: on the limit: x = 80, y = 80, x = w2-4, debug_maps on": dict(
        keypoints=[(400.0, 320.0, 2, B2), (320.0, 400.0, 2, B2), (432.0, 400.0, 2, 0)], score=[], nms=[]),
    "InFrame/level 2: one step outside: x = 79, y = 79, debug_maps on": dict(keypoints=[], score=[], nms=[]),
    "cell index/cell 1, level 1: x = 208 | 209, y = 208 | 209": dict(
        keypoints=[(416.0, 80.0, 1, B1), (436.0, 416.0, 1, B1), (80.0, 418.0, 1, B1), (418.0, 436.0, 1, B1)], score=[], nms=[]),
    "cell index/cell 3, level 1: x = 208 | 209, y = 208 | 209": dict(
        keypoints=[(416.0, 80.0, 1, B1), (436.0, 416.0, 1, B1), (80.0, 418.0, 1, B1), (418.0, 436.0, 1, B1)], score=[], nms=[]),
    "cell index/cell 4, level 1: x = 207 | 208, y = 207 | 208": dict(
        keypoints=[(414.0, 80.0, 1, B1), (436.0, 414.0, 1, B1), (80.0, 416.0, 1, B1), (416.0, 436.0, 1, B1)], score=[], nms=[]),
    "cell index/cell 7, level 1: x = 206 | 207, y = 206 | 207": dict(
        keypoints=[(412.0, 80.0, 1, B1), (436.0, 412.0, 1, B1), (80.0, 414.0, 1, B1), (414.0, 436.0, 1, B1)], score=[], nms=[]),
    "cell index/cell 10, level 1: x = 204 | 205, y = 204 | 205": dict(
        keypoints=[(408.0, 80.0, 1, B1), (436.0, 408.0, 1, B1), (80.0, 410.0, 1, B1), (410.0, 436.0, 1, B1)], score=[], nms=[]),
    "cell index/cell 16, level 1: x = 207 | 208, y = 207 | 208": dict(
        keypoints=[(414.0, 80.0, 1, B1), (436.0, 414.0, 1, B1), (80.0, 416.0, 1, B1), (416.0, 436.0, 1, B1)], score=[], nms=[]),
    "cell index/cell 64, level 1: x = 191 | 192, y = 191 | 192": dict(
        keypoints=[(382.0, 80.0, 1, B1), (436.0, 382.0, 1, B1), (80.0, 384.0, 1, B1), (384.0, 436.0, 1, B1)], score=[], nms=[]),
    "cell index/cell 1, level 2: x = 96 | 97, y = 96 | 97": dict(
        keypoints=[(384.0, 320.0, 2, B2), (424.0, 384.0, 2, B2), (320.0, 388.0, 2, B2), (388.0, 424.0, 2, B2)], score=[], nms=[]),
    "cell index/cell 3, level 2: x = 96 | 97, y = 96 | 97": dict(
        keypoints=[(384.0, 320.0, 2, B2), (424.0, 384.0, 2, B2), (320.0, 388.0, 2, B2), (388.0, 424.0, 2, B2)], score=[], nms=[]),
    "cell index/cell 4, level 2: x = 96 | 97, y = 96 | 97": dict(
        keypoints=[(384.0, 320.0, 2, B2), (424.0, 384.0, 2, B2), (320.0, 388.0, 2, B2), (388.0, 424.0, 2, B2)], score=[], nms=[]),
    "cell index/cell 7, level 2: x = 96 | 97, y = 96 | 97": dict(
        keypoints=[(384.0, 320.0, 2, B2), (424.0, 384.0, 2, B2), (320.0, 388.0, 2, B2), (388.0, 424.0, 2, B2)], score=[], nms=[]),
    "cell index/cell 10, level 2: x = 94 | 95, y = 94 | 95": dict(
        keypoints=[(376.0, 320.0, 2, B2), (424.0, 376.0, 2, B2), (320.0, 380.0, 2, B2), (380.0, 424.0, 2, B2)], score=[], nms=[]),
    "cell index/cell 16, level 2: x = 95 | 96, y = 95 | 96": dict(
        keypoints=[(380.0, 320.0, 2, B2), (424.0, 380.0, 2, B2), (320.0, 384.0, 2, B2), (384.0, 424.0, 2, B2)], score=[], nms=[]),
    "cell index/cell 64, level 2: x = 95 | 96, y = 95 | 96": dict(
        keypoints=[(380.0, 320.0, 2, B2), (424.0, 380.0, 2, B2), (320.0, 384.0, 2, B2), (384.0, 424.0, 2, B2)], score=[], nms=[]),
    "occupied/cell 10, 208 x 136: the neighbours flagged": dict(keypoints=_OCC_UNIT, score=[], nms=[]),
    "occupied/cell 10, 208 x 136: no mask": dict(keypoints=_OCC_UNIT, score=[], nms=[]),
    "occupied/cell 3, 208 x 136: the neighbours flagged": dict(keypoints=_OCC_UNIT, score=[], nms=[]),
    "occupied/cell 3, 208 x 136: no mask": dict(keypoints=_OCC_UNIT, score=[], nms=[]),
    "occupied/cell 4, 448 x 448: the neighbours flagged": dict(keypoints=_OCC_LEVEL2, score=[], nms=[]),
    "occupied/cell 4, 448 x 448: no mask": dict(keypoints=_OCC_LEVEL2, score=[], nms=[]),
    "occupied/cell 3, 448 x 448: the neighbours flagged": dict(keypoints=_OCC_LEVEL2, score=[], nms=[]),
    "occupied/cell 3, 448 x 448: no mask": dict(keypoints=_OCC_LEVEL2, score=[], nms=[]),
    "cell winner/level 1 strictly greater than level 0 replaces it": dict(keypoints=[(108.0, 90.0, 1, B1)], score=[], nms=[]),
    "cell winner/tie at 0.0 across levels 1 and 2 in one cell: both levels": dict(keypoints=[(438.0, 330.0, 1, 0)], score=[], nms=[]),
    "cell winner/tie at 0.0 across levels 1 and 2 in one cell: level 2 alone": dict(keypoints=[(428.0, 368.0, 2, 0)], score=[], nms=[]),
    "cell winner/tie at 0.0 across levels 1 and 2 in one cell: level 1 alone": dict(keypoints=[(438.0, 330.0, 1, 0)], score=[], nms=[]),
    "cell winner/the only candidate of a cell scores 0.0": dict(keypoints=[(198.0, 100.0, 1, 0)], score=[], nms=[]),
    "Shi-Tomasi window/level 1: the window just fits, x = w1-6, y = h1-6": dict(
        keypoints=[(196.0, 90.0, 1, B1), (120.0, 124.0, 1, B1)], score=[], nms=[]),
    "Shi-Tomasi window/level 1: one pixel further out, x = w1-5, y = h1-5": dict(
        keypoints=[(198.0, 90.0, 1, 0), (120.0, 126.0, 1, 0)], score=[], nms=[]),
    "Shi-Tomasi window/level 2: the window just fits, x = w2-6, y = h2-6": dict(
        keypoints=[(424.0, 340.0, 2, B2), (340.0, 424.0, 2, B2)], score=[], nms=[]),
    "Shi-Tomasi window/level 2: one pixel further out, x = w2-5, y = h2-5": dict(
        keypoints=[(428.0, 340.0, 2, 0), (340.0, 428.0, 2, 0)], score=[], nms=[]),
    "output/cell order, px = x * 2^L, the count: cell 1": dict(keypoints=_OUT_FINE, score=[], nms=[]),
    "output/cell order, px = x * 2^L, the count: cell 2": dict(keypoints=_OUT_FINE, score=[], nms=[]),
    "output/cell order, px = x * 2^L, the count: cell 10": dict(
        keypoints=[_OUT_FINE[i] for i in (1, 0, 2, 4, 3, 5, 6, 7, 8, 9, 10)], score=[], nms=[]),
    "output/cell order, px = x * 2^L, the count: cell 64": dict(
        keypoints=[_OUT_FINE[i] for i in (1, 3, 6, 5, 8, 10)], score=[], nms=[]),
    "level 3/x = 160 | 159, y = 159, the window at w3-5": dict(
        keypoints=[(700.0, 700.0, 0, D25), (1280.0, 1304.0, 3, B2), (1368.0, 1368.0, 3, 0)], score=[], nms=[]),
}


def cases():
    if not _cases:
        for build in (_fast_test, _fast_score, _fast_border, _nms, _inframe, _cell_index, _occupied, _winner, _shi_window, _output, _level3):
            build()
    return list(_cases)
