"""CPU checks of the crafted BoW cases of tests/bow_cases.py, which tests/test_gpu_bow.py runs on the kernels of csrc/bow.hip.
Two things are shown for every rule of the descent, of SearchByBoW, of SearchForTriangulation and of the orientation histogram:
the oracle (oracle/bow.c) equals a numpy restatement on the case, and the case DISCRIMINATES: the named wrong variant of the rule, computed
in numpy, gives another answer than the oracle on at least one row.  These are conditions on the cases, not measurements."""
import numpy as np
import pytest
import bow_cases as bc
import fixtures
from oracle.pyoracle import Camera
from test_oracle_bow import _parse, _descend

F32 = np.float32
LEVELSUP = (0, 1, 2, 3, 4, 6)


# ------------------------------------------------------------------------------------------------------------- restatements
def transform_witness(blob, desc, levelsup, **variant):
    _, L, nodes = _parse(blob)
    out = [_descend(nodes, L, d, levelsup, **variant) for d in desc]
    word, weight, node = (np.array([o[i] for o in out]) for i in range(3))
    return word, weight, np.where((weight > 0) & (word >= 0), node, -1)


def search_witness(p, th_low, ratio, le_th=False, double_ratio=False, last_tie=False):
    """Matcher::SearchByBoW (Matcher.cpp:196-292) per row of frame 1; the keywords select the wrong variants"""
    D = bc.hamming(p["d1"], p["d2"])
    out = np.full(len(p["d1"]), -1)
    for i in range(len(out)):
        if p["n1"][i] < 0:
            continue
        b1, b2, idx = 256, 256, -1
        for j in np.nonzero(p["n2"] == p["n1"][i])[0]:
            d = int(D[i, j])
            if d < b1 or (last_tie and d == b1):
                b1, b2, idx = d, b1, j
            elif d < b2:
                b2 = d
        if idx < 0 or not (b1 <= th_low if le_th else b1 < th_low):
            continue
        prod = np.float64(F32(ratio)) * np.float64(b2) if double_ratio else F32(ratio) * F32(b2)
        if np.float64(b1) < np.float64(prod):
            out[i] = idx
    return out


def triangulation_witness(p, th_low, eps, cam=bc.CAM, lt_th=False, first_tie=False, all_double=False, no_den=False):
    """Matcher::SearchForTriangulation (Matcher.cpp:86-193) + CheckDistEpipolarLine (:338-354)"""
    D = bc.hamming(p["d1"], p["d2"])
    out = np.full(len(p["d1"]), -1)
    for i in range(len(out)):
        if p["n1"][i] < 0:
            continue
        js = np.nonzero(p["n2"] == p["n1"][i])[0]
        den, dsqr = bc.epipolar_terms(p["px1"][i], p["px2"][js], p["E"], cam, all_double)
        best = 256
        for t, j in enumerate(js):
            d = int(D[i, j])
            if (d >= th_low if lt_th else d > th_low) or (d >= best if first_tie else d > best):
                continue
            if not no_den and den[t] < 1e-6:
                continue
            if dsqr[t] < eps:
                best, out[i] = d, j
    return out


def orientation_witness(a1, a2, m, floor_bin=False, ge_scan=False, double_tenth=False):
    """the checkOrientation part of Matcher::SearchByBoW (Matcher.cpp:247-256, 271-289) + ComputeThreeMaxima (:293-336)"""
    m = np.asarray(m)
    rot = (np.asarray(a1, np.float64) - np.asarray(a2, np.float64)[np.maximum(m, 0)] if len(a2) else np.zeros(len(m))).astype(F32)
    rot = np.where(rot < 0, rot + F32(360), rot).astype(F32)
    x = (rot * F32(1.0 / 30)).astype(F32).astype(np.float64)
    b = (np.floor(x) if floor_bin else np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(int)          # C round(): half away from zero
    b[b == 30] = 0
    h = np.bincount(b[(m >= 0) & (b >= 0) & (b < 30)], minlength=30)             # a bin outside the histogram (the reference asserts): not counted
    mx, ix = [0, 0, 0], [-1, -1, -1]
    gt = (lambda s, t: s >= t) if ge_scan else (lambda s, t: s > t)
    for i in range(30):
        s = int(h[i])
        if gt(s, mx[0]):
            mx, ix = [s, mx[0], mx[1]], [i, ix[0], ix[1]]
        elif gt(s, mx[1]):
            mx, ix = [mx[0], s, mx[1]], [ix[0], i, ix[1]]
        elif gt(s, mx[2]):
            mx[2], ix[2] = s, i
    tenth = np.float64(F32(0.1)) * mx[0] if double_tenth else np.float64(F32(0.1) * F32(mx[0]))
    if mx[1] < tenth:
        ix[1] = ix[2] = -1
    elif mx[2] < tenth:
        ix[2] = -1
    return int(sum(h[i] for i in set(ix) if i >= 0)), h, ix


def _cam(c=bc.CAM):
    return Camera(*c)


# -------------------------------------------------------------------------------------------------------------- vocabularies
def test_ragged_vocabulary_has_what_it_promises():
    blob, meta = bc.ragged_vocabulary(meta=True)
    k, L, nodes = _parse(blob)
    assert (k, L, len(nodes)) == (4, 4, meta["n_nodes"]) and meta["children"] == [1, 2, 4]
    assert all(0 <= nd["parent"] < i for i, nd in enumerate(nodes) if i)                      # parents before their children
    depth = [0] * len(nodes)
    for i in range(1, len(nodes)):
        depth[i] = depth[nodes[i]["parent"]] + 1
    assert all(bool(nd["leaf"]) == (not nd["children"]) for nd in nodes[1:])
    assert {depth[i] for i in range(1, len(nodes)) if nodes[i]["leaf"]} == {1, 2, 3, 4}
    assert {depth[i] for i in range(1, len(nodes)) if nodes[i]["leaf"] and nodes[i]["w"] == 0} >= {2, 3, 4}
    ties = [nd for nd in nodes if len(nd["children"]) > 1 and np.array_equal(nodes[nd["children"][0]]["desc"], nodes[nd["children"][1]]["desc"])]
    assert len(ties) == 2
    assert any(nodes[nd["children"][-1]]["parent"] != nodes[nd["children"][-1] - 1]["parent"] for nd in nodes if len(nd["children"]) > 1)   # a far sibling
    assert meta["tie_first"] and meta["tie_second"] and not meta["tie_first"] & meta["tie_second"]
    assert all(meta["shallow"][d] for d in (1, 2, 3)) and meta["stopped"]
    # deterministic; the twin differs in nothing but the record size and the padding
    assert bc.ragged_vocabulary() == blob and bc.ragged_vocabulary(seed=8) != blob
    twin = bc.ragged_vocabulary(size_node=48)
    assert len(twin) == 24 + 48 * (len(nodes) - 1)
    n48 = _parse(twin)[2]
    assert all(a["parent"] == b["parent"] and np.array_equal(a["desc"], b["desc"]) and a["w"] == b["w"] and a["leaf"] == b["leaf"] for a, b in zip(nodes, n48))


def test_transform_on_ragged_padded_balanced_and_empty_vocabularies(oracle):
    blob, meta = bc.ragged_vocabulary(meta=True)
    twin = bc.ragged_vocabulary(size_node=48)
    desc = bc.vocabulary_features(blob, 600, 21)
    vo, vt = oracle.vocab_parse(blob), oracle.vocab_parse(twin)
    assert (vo.k, vo.L, vo.n_nodes, vo.n_words) == (4, 4, meta["n_nodes"], meta["n_words"]) == (vt.k, vt.L, vt.n_nodes, vt.n_words)
    tie_differs = leaf_differs = 0
    for levelsup in LEVELSUP:
        word, weight, node = oracle.bow_transform(vo, desc, levelsup)[:3]
        w2, wt2, nd2 = transform_witness(blob, desc, levelsup)
        assert np.array_equal(word, w2) and np.array_equal(weight, wt2) and np.array_equal(node, nd2), levelsup
        t = oracle.bow_transform(vt, desc, levelsup)[:3]
        assert np.array_equal(word, t[0]) and np.array_equal(weight, t[1]) and np.array_equal(node, t[2]), levelsup
        # the cases reach what they were built for
        assert np.isin(word, list(meta["tie_first"])).sum() > 0 and np.isin(word, list(meta["tie_second"])).sum() == 0
        for d in (1, 2, 3):
            assert np.isin(word, meta["shallow"][d]).sum() > 0, d
        assert np.isin(word, meta["stopped"]).sum() > 0 and np.all(node[np.isin(word, meta["stopped"])] == -1)
        if levelsup >= 4:
            assert np.all(node[weight > 0] == 0)                                               # the root
        # wrong variants
        v = transform_witness(blob, desc, levelsup, tie_last=True)
        tie_differs += int((v[0] != word).sum() > 0)
        v = transform_witness(blob, desc, levelsup, shallow_leaf_id=True)
        assert np.array_equal(v[0], word)
        leaf_differs += int((v[2] != node).sum() > 0)
    assert tie_differs == len(LEVELSUP)                                                        # last minimum instead of first
    assert leaf_differs == 3                                                                   # leaf id instead of root: levelsup 0, 1, 2
    # shallow leaves with a positive weight carry the root at levelsup 0
    word, weight, node = oracle.bow_transform(vo, desc, 0)[:3]
    sh = np.isin(word, sum(meta["shallow"].values(), [])) & (weight > 0)
    assert sh.sum() > 0 and np.all(node[sh] == 0) and np.all(node[~sh & (weight > 0)] > 0)
    # balanced k = 3, L = 6
    bal = fixtures.synthetic_vocabulary(k=3, L=6, seed=9)
    vb = oracle.vocab_parse(bal)
    db = bc.vocabulary_features(bal, 257, 22)
    for levelsup in LEVELSUP:
        word, weight, node = oracle.bow_transform(vb, db, levelsup)[:3]
        w2, wt2, nd2 = transform_witness(bal, db, levelsup)
        assert np.array_equal(word, w2) and np.array_equal(weight, wt2) and np.array_equal(node, nd2), levelsup
    # a vocabulary of the root alone (the reference would index an empty vector): word -1, weight 0, node -1
    ve = oracle.vocab_parse(bc.root_only_vocabulary())
    assert (ve.n_nodes, ve.n_words) == (1, 0)
    word, weight, node, bw, bv = oracle.bow_transform(ve, desc[:40], 2)
    assert np.all(word == -1) and np.all(weight == 0) and np.all(node == -1) and len(bw) == 0
    w2, wt2, nd2 = transform_witness(bc.root_only_vocabulary(), desc[:40], 2)
    assert np.array_equal(word, w2) and np.array_equal(node, nd2)
    for name, bad in bc.invalid_vocabularies().items():
        if name in ("L 0", "L 11", "k 0"):
            continue                                    # limits of the GPU loader (ygz_hip_vocab_load); the oracle does not look at k and L
        with pytest.raises(ValueError):
            oracle.vocab_parse(bad)


# ------------------------------------------------------------------------------------------------------------ SearchByBoW
@pytest.fixture(scope="module")
def boundary():
    return bc.match_problem(bc.boundary_rows(), 31)


def test_exact_distances_and_ratio_sweep(boundary):
    p = boundary
    D = bc.hamming(p["d1"], p["d2"])
    assert len(p["d1"]) >= 257 and len(p["d2"]) > 256
    for i, r in enumerate(p["rows"]):
        assert list(D[i, p["owner"] == i]) == list(r), i                                    # the prescribed distances, in frame-2 order
        assert np.all(p["n2"][p["owner"] == i] == p["n1"][i]) and (p["n2"] == p["n1"][i]).sum() == len(r)
    a = np.array([[1, 2, 3] + [0] * 29], np.uint8)
    assert bc.hamming(a, bc.flip_bits(a[0], [0, 9, 255])[None])[0, 0] == 3 and bc.flip_bits(a[0], [0, 9, 255])[[0, 1, 31]].tolist() == [0, 0, 128]
    t = bc.ratio_triples()
    assert len(t) == 84 and (0.6, 3, 5) in t and {r for r, _, _ in t} == {0.6, 0.8}
    # (0.6f, 3, 5): the float product is 3.0 and rejects, the double product 3.0000001 accepts
    assert not F32(3) < F32(0.6) * F32(5) and 3.0 < np.float64(F32(0.6)) * 5.0
    # with 0.9f (the reference default), 0.7f and 0.75f NO pair of distances separates the float product from the double one
    assert bc.ratio_triples((0.9, 0.7, 0.75)) == []


@pytest.mark.parametrize("ratio", [0.6, 0.7, 0.8, 0.9, 1.5])
def test_search_by_bow_boundaries(oracle, boundary, ratio):
    p = boundary
    le = dr = lt = 0
    for th in bc.TH_LOWS:
        m, cnt = oracle.search_by_bow(p["d1"], p["n1"], p["d2"], p["n2"], th, ratio)
        w = search_witness(p, th, ratio)
        assert np.array_equal(m, w) and cnt == (w >= 0).sum(), (th, ratio)
        for i, r in enumerate(p["rows"]):                                   # the rule itself, from the prescribed distances
            if len(r) == 1:
                assert (m[i] >= 0) == (r[0] < th and F32(r[0]) < F32(ratio) * F32(256)), (i, r, th)
            if len(r) == 2 and r[0] != r[1]:
                b1, b2 = min(r), max(r)
                ok = b1 < th and F32(b1) < F32(ratio) * F32(b2)
                assert m[i] == (np.nonzero(p["owner"] == i)[0][int(np.argmin(r))] if ok else -1), (i, r, th)
        le += int(not np.array_equal(search_witness(p, th, ratio, le_th=True), m)) if th < 256 else 0
        dr += int(not np.array_equal(search_witness(p, th, ratio, double_ratio=True), m))
        lt += int(not np.array_equal(search_witness(p, th, ratio, last_tie=True), m))
    assert le == 4                                                          # `<=` instead of `<`: seen at th_low 0, 1, 50, 65
    assert (dr > 0) == (ratio in (0.6, 0.8))                                # the double product: seen where the sweep found triples
    assert (lt > 0) == (ratio > 1)                                          # the last of equal bests: only a ratio above 1 lets a tie through


@pytest.mark.parametrize("shape", bc.MATCH_SHAPES[::3] + [(300, 300)])
def test_search_by_bow_related_sets(oracle, shape):
    p = bc.related_sets(*shape, seed=100 + shape[0])
    m, cnt = oracle.search_by_bow(p["d1"], p["n1"], p["d2"], p["n2"], 65, 0.7)
    w = search_witness(p, 65, 0.7)
    assert np.array_equal(m, w) and cnt == (w >= 0).sum()
    if min(shape) >= 63:
        assert cnt > shape[0] // 8 and (p["n1"] < 0).any() and (p["n2"] < 0).any() and (p["n1"] >= bc.NODE_HI - 1).any()
    one = dict(p, n1=np.full(shape[0], 5, np.int32), n2=np.full(shape[1], 5, np.int32))          # all rows in one node
    m, cnt = oracle.search_by_bow(one["d1"], one["n1"], one["d2"], one["n2"], 65, 0.7)
    assert np.array_equal(m, search_witness(one, 65, 0.7))


# ------------------------------------------------------------------------------------------------- SearchForTriangulation
def test_threshold_placement():
    for eps in (1e-4, 1e-2):
        lo, hi = bc.float_neighbours(eps)
        assert np.float64(lo) < eps <= np.float64(hi) and np.nextafter(lo, F32(1)) == hi
        p = bc.epipolar_problem([[(10, "under")], [(10, "over")], [(10, "on")], [(10, "off")]], eps, 5)
        assert list(p["dsqr"][:2]) == [np.float64(lo), np.float64(hi)] and p["dsqr"][2] < 1e-12 and p["dsqr"][3] > eps
    lo, hi = bc.den_scales()
    assert np.float64(F32(lo) * F32(lo)) < 1e-6 <= np.float64(F32(hi) * F32(hi)) and np.nextafter(F32(lo), F32(1)) == F32(hi)


@pytest.mark.parametrize("eps", [1e-4, 1e-2])
@pytest.mark.parametrize("th", [50, 65])
def test_triangulation_rules(oracle, eps, th):
    p = bc.epipolar_problem(bc.epipolar_rows(th), eps, 41)
    m, cnt = oracle.search_for_triangulation(p["d1"], p["n1"], p["px1"], p["d2"], p["n2"], p["px2"], p["E"], th, eps, cam=_cam())
    w = triangulation_witness(p, th, eps)
    assert np.array_equal(m, w) and cnt == (w >= 0).sum()
    own = lambda i: list(np.nonzero(p["owner"] == i)[0])
    # the replacement rule, both directions (rows 0 .. 3 of epipolar_rows), and the threshold kinds
    assert m[0] == own(0)[1] and m[1] == own(1)[0] and m[2] == own(2)[1] and m[3] == own(3)[2] and m[4] == own(4)[0] and m[5] == own(5)[1]
    assert m[7] == own(7)[1] and m[8] == own(8)[0] and m[9] == own(9)[0] and m[10] == -1 and m[11] >= 0 and m[12] == -1 and m[13] == -1
    for name in ("lt_th", "first_tie", "all_double"):                       # `<` for `<=`; first for last; the all-double evaluation
        assert not np.array_equal(triangulation_witness(p, th, eps, **{name: True}), m), name
    # other intrinsics give another answer on the same pixels: the camera matters
    m2, _ = oracle.search_for_triangulation(p["d1"], p["n1"], p["px1"], p["d2"], p["n2"], p["px2"], p["E"], th, eps)
    assert not np.array_equal(m2, m)


def test_triangulation_den_branch(oracle):
    rows = [[(20, "on")], [(20, "on"), (20, "off")], [(20, "off")], [(30, "on"), (20, "on")]] * 3
    under, over = bc.den_scales()
    for scale, some in ((under, False), (over, True), (0.0, False), (1.0, True)):
        p = bc.epipolar_problem(rows, 1e-4, 43, scale=scale)
        m, cnt = oracle.search_for_triangulation(p["d1"], p["n1"], p["px1"], p["d2"], p["n2"], p["px2"], p["E"], 65, 1e-4, cam=_cam())
        assert np.array_equal(m, triangulation_witness(p, 65, 1e-4)) and (cnt > 0) == some, scale
        differs = not np.array_equal(triangulation_witness(p, 65, 1e-4, no_den=True), m)
        assert differs == (scale == under), scale                           # the branch removed: seen just under 1e-6 (E = 0: 0 / 0 refuses anyway)


@pytest.mark.parametrize("shape", [(65, 257), (257, 513)])
def test_triangulation_related_sets(oracle, shape):
    p = dict(bc.related_sets(*shape, seed=200 + shape[0]), E=bc.x_translation())
    for eps in (1e-4, 1e-2):
        m, cnt = oracle.search_for_triangulation(p["d1"], p["n1"], p["px1"], p["d2"], p["n2"], p["px2"], p["E"], 65, eps, cam=_cam())
        assert np.array_equal(m, triangulation_witness(p, 65, eps)) and cnt > shape[0] // 8


# ------------------------------------------------------------------------------------------------------------ orientation
@pytest.mark.parametrize("name", list(bc.ORIENTATION_HISTS))
def test_orientation_histograms(oracle, name):
    hist = bc.ORIENTATION_HISTS[name]
    for n1 in (255, 256, 257, 1000):
        if hist.sum() > n1:
            continue
        p = bc.orientation_problem(hist, n1, 50, 7 + n1)
        cnt, h, ind = oracle.bow_orientation(p["a1"], p["a2"], p["m"])
        assert np.array_equal(h, hist), n1                                  # the prescribed histogram
        wc, wh, wi = orientation_witness(p["a1"], p["a2"], p["m"])
        assert (cnt, list(ind)) == (wc, wi) and np.array_equal(h, wh)
    want = {"three-way tie": [2, 5, 7], "tie of second and third": [1, 4, 6], "10 1 1": [3, 0, 8], "10 0 0": [11, -1, -1], "100 10 9": [6, 2, -1],
            "one bin": [0, -1, -1], "tie of first and second": [4, 10, 1], "tenth exactly": [5, 6, -1], "all thirteen": [0, 1, 2]}[name]
    assert list(ind) == want
    ge = orientation_witness(p["a1"], p["a2"], p["m"], ge_scan=True)
    assert (ge[2] != want) == (name in ("three-way tie", "tie of second and third", "tie of first and second", "10 1 1"))    # `>=` in the scan: seen on equal counts
    dbl = orientation_witness(p["a1"], p["a2"], p["m"], double_tenth=True)
    assert (dbl[2] != want) == (name in ("10 1 1", "100 10 9", "tenth exactly"))      # the double 0.1 * max1: max2 = max1 / 10 exactly
    fl = orientation_witness(p["a1"], p["a2"], p["m"], floor_bin=True)
    assert np.array_equal(fl[1], hist) == (name == "one bin")                # floor instead of round (bin 0 alone holds no rotation above x.5)


def test_orientation_edges(oracle):
    rots = np.array(bc.EXACT_ROTATIONS)
    for a2v in (0.0, 200.0):
        a1 = (a2v + rots) % 360.0 if a2v else rots
        a2 = np.full(3, a2v)
        m = np.arange(len(rots), dtype=np.int32) % 3
        cnt, h, ind = oracle.bow_orientation(a1, a2, m)
        wc, wh, wi = orientation_witness(a1, a2, m)
        assert (cnt, list(ind)) == (wc, wi) and np.array_equal(h, wh) and h.sum() == len(rots)
    assert [int(np.nonzero(oracle.bow_orientation(rots[i:i + 1], np.zeros(1), np.zeros(1, np.int32))[1])[0][0]) for i in range(5)] == [0, 1, 2, 12, 12]
    for n1, n2 in ((1, 0), (257, 0), (1000, 5)):                            # nothing matched
        p = bc.orientation_problem(np.zeros(30, int), n1, n2, 3)
        cnt, h, ind = oracle.bow_orientation(p["a1"], p["a2"] if n2 else np.zeros(1), p["m"])
        assert cnt == 0 and h.sum() == 0 and list(ind) == [-1, -1, -1]
    a1, a2, m = bc.OUTSIDE_ROTATIONS                                       # angles outside [0, 360): bins outside the histogram are dropped
    cnt, h, ind = oracle.bow_orientation(a1, a2, m)
    wc, wh, wi = orientation_witness(a1, a2, m)
    assert (cnt, list(ind)) == (wc, wi) and np.array_equal(h, wh) and (cnt, list(ind), int(h.sum())) == (4, [12, 0, 1], 4)
    p = bc.orientation_problem(bc.hist30(b9=1), 1, 1, 4)                    # one row
    cnt, h, ind = oracle.bow_orientation(p["a1"], p["a2"], p["m"])
    assert (cnt, list(ind)) == (1, [9, -1, -1])
