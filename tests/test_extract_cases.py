"""CPU checks of the crafted extractor cases of tests/extract_cases.py, which tests/test_gpu_extract_limits.py runs on k_fast_select, k_compact
and k_describe.  For every case three things are shown: the oracle (fast_detect, fast_score, fast_nonmax, shi_tomasi, detect) gives the
case's LITERALS; a numpy witness, written here from the rule table of DESIGN.md section 38 and not from oracle/orb.c, gives the same
keypoints (position, level, score bits) and the same maps; and the cases DISCRIMINATE: for every wrong variant of a rule (a strict comparison
written as a closed one, an arc of nine, a cell index without the level's scale, ...) the witness run with that variant departs from the
literals on at least one case of the rule's row.  A variant that no case can tell apart fails the test: the rule would not be covered.
No case is marked or skipped, and every comparison is an equality."""
import numpy as np
import pytest

import extract_cases as ec

F32 = np.float32


# ==== the witness ==========================================================================================================
def _arc(flags, n):
    """flags [16, ...]: some n ring positions in a row on the circle are all set (brute force over the sixteen starts)"""
    out = np.zeros(flags.shape[1:], bool)
    for s in range(16):
        run = flags[s]
        for k in range(1, n):
            run = run & flags[(s + k) % 16]
        out |= run
    return out


def witness_fast(img, thr, v=None):
    """steps 1 and 2: the stored score map (score + 1, 0 where there is no corner)"""
    h, w = img.shape
    c = img.astype(np.int16)
    pad = np.pad(c, 3, mode="edge")                                          # only a variant's wider domain reads the padding
    ring = np.stack([pad[3 + dy:3 + dy + h, 3 + dx:3 + dx + w] for dx, dy in ec.RING])
    n = 9 if v == "arc9" else 10

    def corner(r, p, t):
        if v == "thr_ge":
            return _arc(r >= p + t, n) | _arc(r <= p - t, n)
        return _arc(r > p + t, n) | _arc(r < p - t, n)
    b = 2 if v == "border2" else 3
    cand = np.zeros((h, w), bool)
    cand[b:h - b, b:w - b] = (np.abs(ring - c).max(axis=0) >= max(thr, 1))[b:h - b, b:w - b]      # a flat neighbourhood is no corner: skip it
    ys, xs = np.nonzero(cand)
    r, p = ring[:, ys, xs], c[ys, xs]
    is_c = corner(r, p, thr)
    ys, xs, r, p = ys[is_c], xs[is_c], r[:, is_c], p[is_c]
    score = np.full(len(p), thr, np.int64)
    for t in range(thr + 1, 255):                                            # the largest threshold that still passes
        ok = corner(r, p, t)
        if not ok.any():
            break
        score[ok] = t
    smap = np.zeros((h, w), np.uint8)
    smap[ys, xs] = score + 1
    return smap


def witness_nms(smap, tie, v=None):
    """step 3 on the stored scores"""
    if v == "nms_tie_flipped":
        tie = 1 - tie
    s = np.pad(smap.astype(np.int16), 1)
    h, w = smap.shape
    keep = smap > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dx, dy) == (0, 0) or (v == "nms_4_neighbours" and dx != 0 and dy != 0):
                continue
            o = s[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
            keep &= ~((o >= smap) if tie else (o > smap))
    return keep.astype(np.uint8)


def witness_shi(img, x, y, v=None):
    """step 7, in the float order of the table"""
    h, w = img.shape
    out = (x - 4 < 1 or x + 4 > w - 1 or y - 4 < 1 or y + 4 > h - 1) if v == "shi_window_closed" else \
          (x - 4 < 1 or x + 4 >= w - 1 or y - 4 < 1 or y + 4 >= h - 1)
    if out:
        return F32(0.0)
    a = np.pad(img.astype(np.int64), 8)                                      # only a variant's window reads the padding
    y0, x0 = y + 8 - 4, x + 8 - 4
    gx = a[y0:y0 + 8, x0 + 1:x0 + 9] - a[y0:y0 + 8, x0 - 1:x0 + 7]
    gy = a[y0 + 1:y0 + 9, x0:x0 + 8] - a[y0 - 1:y0 + 7, x0:x0 + 8]
    dxx, dyy, dxy = (F32(int((p * q).sum()) / 128.0) for p, q in ((gx, gx), (gy, gy), (gx, gy)))
    tr = F32(dxx + dyy)
    disc = F32(F32(tr * tr) - F32(F32(4.0) * F32(F32(dxx * dyy) - F32(dxy * dxy))))
    return F32(0.5 * float(F32(tr - np.sqrt(disc))))


def witness(levels, params, occupied=None, v=None):
    """steps 1-9: dict(keypoints [(px, py, level, score bits)], score [map per level], nms [map per level])"""
    cell, thr, tie = params["cell_size"], params["fast_threshold"], params["nms_tie_suppress"]
    rows0, cols0 = levels[0].shape
    gcols, grows = -(-cols0 // cell), -(-rows0 // cell)
    smaps = [witness_fast(im, thr, v) for im in levels]
    nmaps = [witness_nms(s, tie, v) for s in smaps]
    best = {}
    order = range(len(levels) - 1, -1, -1) if v == "levels_descending" else range(len(levels))
    for L in order:
        s = 1 << L
        ys, xs = np.nonzero(nmaps[L])                                        # raster order: rows, then columns
        if v == "raster_x_major":
            o = np.lexsort((ys, xs))
            ys, xs = ys[o], xs[o]
        for x, y in zip(xs.tolist(), ys.tolist()):
            if v == "inframe_divided_once":
                inside = 20 <= x < cols0 - 20 and 20 <= y < rows0 - 20
            else:
                lo = (lambda a: a > 20 * s) if v == "inframe_lo_gt" else (lambda a: a >= 20 * s)
                hi = (lambda a, n: a <= (n - 20) * s) if v == "inframe_hi_le" else (lambda a, n: a < (n - 20) * s)
                inside = lo(x) and lo(y) and hi(x, cols0) and hi(y, rows0)
            if not inside:
                continue
            if v == "cell_without_scale":
                gx, gy = x // cell, y // cell
            elif v == "cell_rounded":
                gx, gy = (2 * x * s + cell) // (2 * cell), (2 * y * s + cell) // (2 * cell)
            else:
                gx, gy = (x * s) // cell, (y * s) // cell
            k = gy * gcols + gx
            if k < 0 or k >= gcols * grows:
                continue
            if occupied is not None and occupied[k] and (L == 0 or v != "occupied_level0_only"):
                continue
            sc = witness_shi(levels[L], x, y, v)
            if v == "zero_score_dropped" and sc == 0:
                continue
            if k in best and not (sc >= best[k][3] if v == "replace_ge" else sc > best[k][3]):
                continue
            best[k] = (float(x * s), float(y * s), L, sc)
    kps = [(b[0], b[1], b[2], int(b[3].view(np.uint32))) for _, b in sorted(best.items())]
    return dict(keypoints=kps, score=smaps, nms=nmaps)


VARIANTS = [(v, row) for row, vs in (
    ("FAST test", ("thr_ge", "arc9")),
    ("FAST border", ("border2",)),
    ("NMS", ("nms_tie_flipped", "nms_4_neighbours")),
    ("InFrame", ("inframe_lo_gt", "inframe_hi_le", "inframe_divided_once")),
    ("cell index", ("cell_without_scale", "cell_rounded")),
    ("occupied", ("occupied_level0_only",)),
    ("cell winner", ("replace_ge", "levels_descending", "raster_x_major", "zero_score_dropped")),
    ("Shi-Tomasi window", ("shi_window_closed",)),
) for v in vs]


# ==== the oracle's side ===========================================================================================================================
def oracle_params(oracle, c):
    h, w = c.picture.shape
    p = oracle.default_params(w, h, c.params["levels"])
    p.cell_size, p.detection_threshold, p.nms_tie_suppress = c.params["cell_size"], float(c.params["fast_threshold"]), c.params["nms_tie_suppress"]
    return p


def oracle_maps(oracle, img, thr, tie):
    xy = oracle.fast_detect(img, thr)
    sc = oracle.fast_score(img, xy, thr)
    nm = oracle.fast_nonmax(xy, sc, tie)
    smap, nmap = np.zeros(img.shape, np.uint8), np.zeros(img.shape, np.uint8)
    smap[xy[:, 1], xy[:, 0]] = sc + 1
    nmap[xy[nm, 1], xy[nm, 0]] = 1
    return smap, nmap


def as_tuples(k):
    return [(float(a), float(b), int(l), int(s)) for a, b, l, s in zip(k["px"], k["py"], k["level"], k["score"].view(np.uint32))]


@pytest.fixture(scope="module")
def pyramids(oracle):
    """case name -> its levels, built once"""
    return {c.name: oracle.pyramid(c.picture, c.params["levels"]) for c in ec.cases()}


# ==== the tests ===================================================================================================================================
def test_every_row_has_cases_on_and_off_its_limit():
    cases = ec.cases()
    assert {c.row for c in cases} == set(ec.ROWS) and all(c.expected is not None for c in cases)
    assert len({c.name for c in cases}) == len(cases)
    for row, on, off in (("FAST test", "on", "outside"), ("FAST border", "3", "2"), ("NMS", "equal", "stronger by 1"), ("InFrame", "on the limit", "outside"),
                         ("cell index", "|", "|"), ("occupied", "flagged", "neighbours"), ("cell winner", "tie", "stronger"),
                         ("Shi-Tomasi window", "just fits", "further out")):
        names = [c.name for c in cases if c.row == row]
        assert any(on in n for n in names) and any(off in n for n in names), row
    # the sizes and parameters the rows are meant to reach
    assert {c.picture.shape[::-1] for c in cases} == {ec.UNIT, ec.TWIN, ec.LEVEL2, ec.LEVEL3}
    assert {c.params["fast_threshold"] for c in cases} == {0, 1, 15, 40, 254}
    assert {c.params["cell_size"] for c in cases} == {1, 2, 3, 4, 7, 10, 16, 64}
    assert {k[2] for c in cases for k in c.expected["keypoints"]} == {0, 1, 2, 3}               # every level is some keypoint's literal
    assert any(k[3] == 0 for c in cases for k in c.expected["keypoints"])                         # and so is the score 0.0
    assert {s for c in cases for s in c.expected["score"]} >= {0, 1, 2, 16, 41, 255}


def test_the_oracle_gives_the_literals_and_the_witness_agrees(oracle, pyramids):
    for c in ec.cases():
        lv = pyramids[c.name]
        thr, tie = c.params["fast_threshold"], c.params["nms_tie_suppress"]
        maps = [oracle_maps(oracle, im, thr, tie) for im in lv]
        ok_ = as_tuples(oracle.detect(lv, oracle_params(oracle, c), c.occupied))
        assert ec.holds(c, ok_, [m[0] for m in maps], [m[1] for m in maps]) == [], c.name
        w = witness(lv, c.params, c.occupied)
        assert ec.holds(c, w["keypoints"], w["score"], w["nms"]) == [], c.name
        for L in range(len(lv)):                                             # the whole maps, not only the probes
            assert np.array_equal(w["score"][L], maps[L][0]) and np.array_equal(w["nms"][L], maps[L][1]), (c.name, L)
        for px, py, L, bits in ok_:                                          # Shi-Tomasi through its own entry point
            assert F32(oracle.shi_tomasi(lv[L], int(px) >> L, int(py) >> L)).view(np.uint32) == bits, c.name


def test_the_designed_premises_hold(oracle, pyramids):
    """what the builders of the bump cases rely on, shown on the pictures: a bump of level L is one corner of level L and none below"""
    for c in ec.cases():
        if c.row in ("InFrame", "Shi-Tomasi window", "cell index", "level 3") and c.params["levels"] > 1:
            lv = pyramids[c.name]
            top = c.params["levels"] - 1
            for L in range(top):
                assert not len(oracle.fast_detect(lv[L], c.params["fast_threshold"])) or c.row == "level 3" and L == 0, (c.name, L)
    by = {c.name: c for c in ec.cases()}
    # FAST border: the corner one step inside is found, the stamp one step outside is not (probes alternate inside | outside)
    for c in ec.cases():
        if c.row == "FAST border":
            assert all(s > 0 for s in c.expected["score"][0::2]) and not any(c.expected["score"][1::2]), c.name
    # Shi-Tomasi window: positive where it fits, the literal 0.0 one pixel further out, the same corners otherwise
    for L in (1, 2):
        fit = next(c for c in ec.cases() if c.row == "Shi-Tomasi window" and "level %d: the window just fits" % L in c.name)
        out = next(c for c in ec.cases() if c.row == "Shi-Tomasi window" and "level %d: one pixel further out" % L in c.name)
        assert len(fit.expected["keypoints"]) == len(out.expected["keypoints"]) == 2
        assert all(k[2] == L and 0 < k[3] < 0x7F800000 for k in fit.expected["keypoints"]) and all(k[2] == L and k[3] == 0 for k in out.expected["keypoints"])
    # the tie at 0.0: either level alone is the cell's keypoint, together level 1 is
    t = {n.split(": ")[-1]: by[n].expected["keypoints"] for n in by if "tie at 0.0" in n}
    assert len(t["level 1 alone"]) == len(t["level 2 alone"]) == 1 and t["both levels"] == t["level 1 alone"]
    assert t["level 1 alone"][0][2:] == (1, 0) and t["level 2 alone"][0][2:] == (2, 0)
    only = by["cell winner/the only candidate of a cell scores 0.0"].expected["keypoints"]
    assert len(only) == 1 and only[0][2:] == (1, 0)
    # InFrame: the cases differ by one pixel and by one keypoint each; debug_maps changes nothing
    for c in ec.cases():
        if c.row == "InFrame" and "debug_maps on" in c.name:
            assert c.expected["keypoints"] == by[c.name.replace("debug_maps on", "debug_maps off")].expected["keypoints"], c.name
            if "one step outside" in c.name:
                assert c.expected["keypoints"] == [], c.name
            elif "on the limit" in c.name:
                assert len(c.expected["keypoints"]) == 3 and all(k[2] == c.params["levels"] - 1 for k in c.expected["keypoints"]), c.name
    # cell index and occupied: every corner is there exactly when its own cell is free
    for c in ec.cases():
        if c.row == "cell index":
            assert len(c.expected["keypoints"]) == 4 and all(k[2] == c.params["levels"] - 1 for k in c.expected["keypoints"]), c.name
        if c.row == "occupied" and "neighbours" in c.name:
            free = by[c.name.replace("the neighbours flagged", "no mask")].expected["keypoints"]
            assert c.expected["keypoints"] == free and {k[2] for k in free} == ({0, 1} if c.picture.shape[::-1] == ec.UNIT else {0, 1, 2}), c.name


@pytest.mark.parametrize("variant,row", VARIANTS)
def test_the_cases_separate_the_wrong_variant(pyramids, variant, row):
    told = []
    for c in ec.cases():
        if c.row == row:
            w = witness(pyramids[c.name], c.params, c.occupied, variant)
            if ec.holds(c, w["keypoints"], w["score"], w["nms"]):
                told.append(c.name)
    assert told, "no case of %r tells %s apart" % (row, variant)


def test_every_variant_of_the_witness_is_in_the_table():
    import inspect
    import re
    src = "".join(inspect.getsource(f) for f in (witness_fast, witness_nms, witness_shi, witness))
    assert set(re.findall(r'v [!=]= "(\w+)"', src)) == {v for v, _ in VARIANTS}
    assert {v for v, _ in VARIANTS} >= {"thr_ge", "arc9", "border2", "nms_tie_flipped", "nms_4_neighbours", "inframe_lo_gt", "inframe_hi_le",
                                        "inframe_divided_once", "cell_without_scale", "cell_rounded", "replace_ge", "levels_descending",
                                        "raster_x_major", "occupied_level0_only", "shi_window_closed", "zero_score_dropped"}


def test_shi_tomasi_window_on_the_low_side(oracle):
    """x - 4 < 1 and y - 4 < 1 cannot be reached through Detect (step 4 keeps x >= 20 * 2^L): through the oracle's own entry point"""
    img = ec.flat((40, 40))
    for x, y in ((4, 20), (5, 20), (20, 4), (20, 5), (34, 20), (35, 20), (20, 34), (20, 35), (5, 5), (4, 4), (34, 34), (35, 35)):
        img[:] = ec.BG
        ec.dot(img, x, y, 25)
        want = 0.0 if (x in (4, 35) or y in (4, 35)) else 25 * 25 / 64.0
        assert oracle.shi_tomasi(img, x, y) == want and float(witness_shi(img, x, y)) == want, (x, y)


def test_the_reciprocal_cell_division_is_exact():
    """the bound the kernel's comment claims (detect.hip, FastArgs::cell_magic): v / cell == (v * ceil(2^32 / cell)) >> 32 for every
    v < 2^16 and every cell size from 2 to 8192"""
    v = np.arange(1 << 16, dtype=np.uint64)
    for cell in range(2, 8193):
        m = np.uint64(((1 << 32) + cell - 1) // cell)
        assert m < (1 << 32) and np.array_equal((v * m) >> np.uint64(32), v // np.uint64(cell)), cell


def test_the_sweep_cannot_pass_vacuously(oracle):
    """every configuration of the GPU sweep, on the CPU: at the unit sizes the oracle returns at least 50 keypoints, and every level that can
    win a cell at that size (20 * 2^L <= w_L - 4: step 4 against step 1's domain) wins at least one"""
    import test_gpu_extract_limits as g
    seen = dict(thr=set(), cell=set(), levels=set(), tie=set(), size=set(), pic=set())
    for cfg in g.SWEEP:
        pic, size, thr, cell, levels, tie = cfg
        img = g.sweep_picture(pic, size)
        assert img.shape[::-1] == size and (thr != 0 or pic == "noise")
        p = oracle.default_params(size[0], size[1], levels)
        p.cell_size, p.detection_threshold, p.nms_tie_suppress = cell, float(thr), tie
        k = oracle.detect(oracle.pyramid(img, levels), p)
        if size in (ec.UNIT, ec.TWIN):
            assert len(k) >= 50, cfg
        can = {L for L in range(levels) if all(20 * 2 ** L <= n - 4 for n in ec.level_size(size, L))}
        assert set(k["level"].tolist()) == can, (cfg, np.bincount(k["level"]))
        for key, val in zip(("pic", "size", "thr", "cell", "levels", "tie"), cfg):
            seen[key].add(val)
    assert seen["thr"] == {0, 7, 15, 40} and seen["cell"] == {1, 3, 4, 10, 16, 64} and seen["levels"] == {1, 2, 3, 5} and seen["tie"] == {0, 1}
    assert seen["size"] == {ec.UNIT, ec.TWIN, (640, 480)} and seen["pic"] == {"texture", "noise"}
    big = [c for c in g.SWEEP if c[1] == (640, 480)]
    assert {c[0] for c in big} == {"texture"} and max(c[4] for c in big) >= 3     # one frame; the interior tiles of levels 1 and 2
