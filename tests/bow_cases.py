"""Crafted cases for the BoW rows (oracle/bow.c, ygz_slam_amd/csrc/bow.hip), shared by tests/test_bow_cases.py (CPU: the oracle against numpy
restatements, and every case against the wrong variant it was built to expose) and tests/test_gpu_bow.py (the kernels against the oracle).
numpy only, fixed seeds, nothing measured: ragged vocabularies in DBoW3's binary format, descriptor sets at exact Hamming distances with
prescribed (best, second best) per row, epipolar problems placed on float boundaries, rotation sets with a prescribed histogram."""
import struct
import numpy as np

LUT = np.array([bin(i).count("1") for i in range(256)])
F32 = np.float32
CAM = (311.5, 287.25, 158.75, 121.5)            # fx, fy, cx, cy: float-representable and not the context's defaults
RATIOS = (0.6, 0.7, 0.75, 0.8, 0.9)            # knnRatio values of the sweep (0.9: the reference default, Matcher.h)
NODE_HI = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------------------- vocabularies
def _pack(nodes, k, L, size_node):
    """nodes: (parent, desc[32], weight, is_leaf) in file order (id = position + 1).  size_node > 41 pads every record with bytes that are
    neither 0 nor 1, so a loader that took is_leaf (or the next parent) from the padding would be seen."""
    out = [struct.pack("<IIiiii", len(nodes), size_node, k, L, 0, 0)]
    for par, desc, w, leaf in nodes:
        out.append(struct.pack("<i", par) + np.asarray(desc, np.uint8).tobytes() + struct.pack("<f", w) + bytes([leaf]) + b"\xa5" * (size_node - 41))
    return b"".join(out)


def ragged_vocabulary(seed=7, size_node=41, k=4, meta=False):
    """A vocabulary tree of L = 4 in DBoW3's binary format (Vocabulary::loadFromBinaryFile) that is NOT balanced: parents with 1, 2 and k
    children, leaves at depths 1, 2, 3 and 4, stopped words (weight 0) at depths 2, 3 and 4, two parents whose first two children carry the
    same descriptor (one pair of inner nodes, one pair of leaves), and one child that stands at the end of the file, far from its siblings.
    Ids are in file order, parents before their children.  The bytes do not depend on size_node except for the padding.
    meta=True also returns what the tests count: words under the first / second child of every tied pair, the words of the shallow leaves by
    depth, the stopped words."""
    rng = np.random.default_rng(seed)
    nodes, depth = [], {0: 0}

    def add(parent, desc, leaf=0, weight=0.0):
        nodes.append([parent, desc, float(F32(weight)), leaf])
        depth[len(nodes)] = depth[parent] + 1
        return len(nodes)

    def near(desc, d):
        return desc ^ np.packbits(rng.random(256) < 0.25 / d)

    def weight(stop=0.1):
        w = float(rng.uniform(0.5, 8.0))
        return 0.0 if rng.random() < stop else w

    def kids(parent, n, leaf=0, stop=0.1, tie=False):
        """n children of `parent`, consecutive in the file"""
        pd = nodes[parent - 1][1] if parent else None
        ids = []
        for c in range(n):
            d = rng.integers(0, 256, 32, dtype=np.uint8) if pd is None else near(pd, depth[parent] + 1)
            if tie and c == 1:
                d = nodes[ids[0] - 1][1].copy()
            ids.append(add(parent, d, leaf, weight(stop) if leaf else 0.0))
        return ids

    A, B, C_, D = kids(0, k)
    nodes[A - 1][2:] = [float(F32(3.25)), 1]                                 # a word at depth 1
    B1, = kids(B, 1)
    B1a, B1b = kids(B1, 2)
    nodes[B1b - 1][2:] = [float(F32(1.5)), 1]                                # a word at depth 3 beside an inner node
    kids(B1a, k, leaf=1)
    C1, C2 = kids(C_, 2)
    nodes[C1 - 1][2:] = [float(F32(2.75)), 1]                                # a word at depth 2
    c2 = kids(C2, k, tie=True)                                               # the first two: same descriptor, both inner nodes
    kids(c2[0], k, leaf=1, stop=0.0); kids(c2[1], k, leaf=1, stop=0.0)
    nodes[c2[2] - 1][2:] = [0.0, 1]                                          # a stopped word at depth 3
    for c in c2[3:]:
        nodes[c - 1][2:] = [float(F32(4.5)), 1]
    tie_pairs = [(c2[0], c2[1])]
    d_kids = kids(D, k)
    for j, g in enumerate(kids(d_kids[0], k)):
        lv = kids(g, k, leaf=1, stop=0.0 if j == 1 else 0.1, tie=(j == 1))   # one pair of leaves with the same descriptor
        if j == 1:
            tie_pairs.append((lv[0], lv[1]))
    for g in kids(d_kids[1], 2):
        kids(g, k, leaf=1)
    nodes[d_kids[2] - 1][2:] = [0.0, 1]                                      # a stopped word at depth 2
    for c in d_kids[3:-1]:
        nodes[c - 1][2:] = [float(F32(5.0)), 1]
    last = d_kids[-1]
    g, = kids(last, 1)
    kids(g, k, leaf=1)
    add(last, near(nodes[last - 1][1], 3), 1, 6.5)                           # its second child, at the end of the file
    blob = _pack(nodes, k, 4, size_node)
    if not meta:
        return blob
    word, parent = {}, {0: -1}
    for i, (par, _, w, leaf) in enumerate(nodes):
        parent[i + 1] = par
        if leaf:
            word[i + 1] = len(word)

    def under(top):
        out = set()
        for nid, w in word.items():
            a = nid
            while a > 0 and a != top:
                a = parent[a]
            if a == top:
                out.add(w)
        return out

    return blob, dict(tie_first=set().union(*[under(a) for a, _ in tie_pairs]), tie_second=set().union(*[under(b) for _, b in tie_pairs]),
                      shallow={d: sorted(w for nid, w in word.items() if depth[nid] == d) for d in (1, 2, 3)},
                      stopped=sorted(w for nid, w in word.items() if nodes[nid - 1][2] == 0.0),
                      children=sorted(set(np.bincount([n[0] for n in nodes]).tolist()) - {0}), n_nodes=len(nodes) + 1, n_words=len(word), k=k)


def root_only_vocabulary(k=4, L=4):
    """no node but the root"""
    return struct.pack("<IIiiii", 0, 41, k, L, 0, 0)


def node_descriptors(blob):
    nb, sz = struct.unpack_from("<II", blob, 0)
    return np.stack([np.frombuffer(blob, np.uint8, 32, 24 + i * sz + 4) for i in range(nb)]) if nb else np.zeros((0, 32), np.uint8)


def vocabulary_features(blob, n, seed):
    """n descriptors for a vocabulary: two in three are node descriptors (inner nodes and leaves) with a few bits flipped, so every branch
    of a ragged tree is walked; the others are uniform noise"""
    rng = np.random.default_rng(seed)
    nd = node_descriptors(blob)
    out = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if len(nd):
        pick = rng.random(n) < 2 / 3
        src = nd[rng.integers(0, len(nd), n)] ^ np.packbits(rng.random((n, 256)) < 0.02, axis=1)
        out[pick] = src[pick]
    return out


def invalid_vocabularies():
    """name -> blob that the loader must refuse"""
    good = ragged_vocabulary()
    nb, = struct.unpack_from("<I", good, 0)

    def header(**kw):
        h = dict(nb=nb, sz=41, k=4, L=4); h.update(kw)
        return struct.pack("<IIiiii", h["nb"], h["sz"], h["k"], h["L"], 0, 0) + good[24:]

    def with_parent(rec, par):
        b = bytearray(good); struct.pack_into("<i", b, 24 + rec * 41, par)
        return bytes(b)

    return {"truncated": good[:-1], "header only": good[:24], "short header": good[:23], "parent of itself": with_parent(9, 10),
            "parent after child": with_parent(9, 30), "negative parent": with_parent(0, -1), "size_node 40": header(sz=40),
            "L 0": header(L=0), "L 11": header(L=11), "k 0": header(k=0)}


# ---------------------------------------------------------------------------------------------------- exact Hamming distances
def flip_bits(row, bits):
    out = np.array(row, np.uint8)
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def at_distance(row, d, rng):
    """a copy of row with exactly d bits flipped"""
    return flip_bits(row, rng.choice(256, int(d), replace=False))


def hamming(a, b):
    return LUT[a[:, None, :] ^ b[None, :, :]].sum(-1)


def ratio_triples(ratios=RATIOS):
    """(ratio, best1, best2) at which `float(best1) < ratio * float(best2)` accepts in double and rejects in float or the reverse: the
    exhaustive sweep over 0 <= best1 < best2 <= 256"""
    out = []
    for r in ratios:
        b1, b2 = np.meshgrid(np.arange(256), np.arange(257), indexing="ij")
        f = b1.astype(F32) < F32(r) * b2.astype(F32)
        d = b1.astype(np.float64) < np.float64(F32(r)) * b2.astype(np.float64)
        out += [(r, int(i), int(j)) for i, j in np.argwhere(f != d) if i < j]
    return out


def match_problem(rows, seed, nodes=None):
    """rows[i] = the Hamming distances of row i's candidates in frame 2, in the order in which they stand there (a value of 256 is not
    possible: an empty list gives a node that frame 2 lacks).  Every row of frame 1 has a node of its own (nodes[i], default 10 + i), so
    (best1, best2) of row i is exactly what rows[i] prescribes.  Frame 2 holds candidate 0 of every row, then candidate 1 of every row, ...:
    with more than 256 rows the candidates of one row lie in different LDS tiles."""
    rng = np.random.default_rng(seed)
    n1 = len(rows)
    nodes = np.arange(10, 10 + n1) if nodes is None else np.asarray(nodes)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2, n2, owner = [], [], []
    for t in range(max([len(r) for r in rows] + [0])):
        for i, r in enumerate(rows):
            if t < len(r):
                d2.append(at_distance(d1[i], r[t], rng)); n2.append(nodes[i]); owner.append(i)
    d2 = np.stack(d2) if d2 else np.zeros((0, 32), np.uint8)
    for i, r in enumerate(rows):                                    # ties are two different descriptors (but for distance 0)
        mine = d2[np.array(owner, int) == i][np.array(r, int) > 0] if len(r) else []
        assert len(mine) < 2 or len(np.unique(mine, axis=0)) == len(mine)
    return dict(d1=d1, n1=nodes.astype(np.int32), d2=d2, n2=np.array(n2, np.int32), owner=np.array(owner, np.int32), rows=rows)


TH_LOWS = (0, 1, 50, 65, 256)


def boundary_rows():
    """the mode-0 boundary problem: th_low - 1, th_low, th_low + 1 for every th_low of TH_LOWS with a far second best, with none (best2 = 256)
    and with a second best that the ratios 0.6 .. 0.9 split; every triple of ratio_triples(); ties of the best (first wins, seen only with
    a ratio above 1), of best and second best, three equal; a node that frame 2 lacks"""
    rows = []
    for th in TH_LOWS:
        for b1 in (th - 1, th, th + 1):
            if 0 <= b1 <= 255:
                rows += [[b1, 255], [b1], [255, b1], [b1, min(255, b1 + b1 // 3 + 1)]]
    rows += [[b1, b2] if b2 < 256 else [b1] for _, b1, b2 in ratio_triples()]
    rows += [[b2, b1] for _, b1, b2 in ratio_triples() if b2 < 256]
    rows += [[40, 40, 90], [90, 40, 40], [40, 90, 40], [40, 40, 40], [0, 0], [0, 1], [0], [255], [255, 255], [30, 40, 40], [40, 30, 30], [],
             [12, 200, 12, 200], [64, 64, 65]]
    rows += [[(7 * i) % 200, (13 * i) % 256, (29 * i) % 97][:1 + i % 3] for i in range(max(0, 300 - len(rows)))]      # past one block and one tile
    return rows


# --------------------------------------------------------------------------------------------------------- epipolar problems
def x_translation(scale=1.0):
    """E = scale * [t]x for t = (1, 0, 0): with line = pt1^T E (Matcher.cpp:341-343) a = 0, b = scale, c = -scale * y1: the image rows"""
    E = np.zeros((3, 3))
    E[1, 2], E[2, 1] = -scale, scale
    return E


def epipolar_terms(p1, p2, E, cam=CAM, all_double=False):
    """CheckDistEpipolarLine (Matcher.cpp:338-354) for one pixel p1 against pixels p2 [m][2], with the float steps of the reference (a, b, c
    floats of double expressions, num a float of a double expression, den and dsqr in float) or, all_double, with none of them.
    Returns (den, dsqr) as float64 arrays."""
    fx, fy, cx, cy = [np.float64(F32(v)) for v in cam]
    E = np.asarray(E, np.float64).reshape(3, 3)
    p2 = np.asarray(p2, np.float64).reshape(-1, 2)
    x1, y1 = (np.float64(p1[0]) - cx) * 1.0 / fx, (np.float64(p1[1]) - cy) * 1.0 / fy
    x2, y2 = (p2[:, 0] - cx) * 1.0 / fx, (p2[:, 1] - cy) * 1.0 / fy
    a, b, c = (x1 * E[0, i] + y1 * E[1, i] + E[2, i] for i in range(3))
    with np.errstate(all="ignore"):
        if all_double:
            den = np.full(len(p2), a * a + b * b)
            num = a * x2 + b * y2 + c
            return den, np.abs(num * num / den)
        a, b, c = F32(a), F32(b), F32(c)
        num = (np.float64(a) * x2 + np.float64(b) * y2 + np.float64(c)).astype(F32)
        den = F32(F32(a * a) + F32(b * b))
        dsqr = ((num * num).astype(F32) / den).astype(F32)
        return np.full(len(p2), np.float64(den)), np.abs(dsqr).astype(np.float64)


def float_neighbours(eps):
    """the largest float below the double eps and the smallest float not below it"""
    f = F32(eps)
    return (np.nextafter(f, F32(0)), f) if np.float64(f) >= eps else (f, np.nextafter(f, F32(np.inf)))


def _floats_around(x, n):
    c = np.array([x], F32).view(np.int32)[0]
    return (c + np.arange(-n, n + 1, dtype=np.int32)).view(F32)


def threshold_scale(eps):
    """(scale, num_under, num_over): an E scale (a float) and two float values of `num` for which dsqr = fl(fl(num * num) / fl(scale^2)) is
    exactly the float below eps and exactly the float above it -- squares of floats skip floats, so the scale is searched"""
    lo, hi = float_neighbours(eps)
    for s in [1.0 + j / 64 for j in range(0, 256)]:
        b = F32(s)
        den = F32(b * b)
        n = _floats_around(np.sqrt(eps * np.float64(den)), 64)
        d = ((n * n).astype(F32) / den).astype(F32)
        u, o = n[d == lo], n[d == hi]
        if len(u) and len(o):
            return float(b), u[0], o[0]
    raise AssertionError("no scale reaches both float neighbours of %g" % eps)


def den_scales():
    """two floats b (adjacent) with fl(b * b) just under and just not under 1e-6: E scales at which CheckDistEpipolarLine's `den < 1e-6`
    (a = 0) refuses and evaluates"""
    n = _floats_around(1e-3, 64)
    den = (n * n).astype(F32).astype(np.float64)
    i = int(np.nonzero(den < 1e-6)[0].max())
    assert den[i] < 1e-6 <= den[i + 1]
    return float(n[i]), float(n[i + 1])


def _v2_for_num(v1, num, scale, cam):
    """the row v2 at which the float `num` of the pixel pair comes out as the given float (a = 0, b = scale, c = float(-scale * y1))"""
    fy, cy = np.float64(F32(cam[1])), np.float64(F32(cam[3]))
    y1 = (np.float64(v1) - cy) * 1.0 / fy
    c = np.float64(F32(y1 * -scale))
    return ((np.float64(num) - c) / scale) * fy + cy


def _disagree_v2(p1, kind, E, eps, cam, s):
    """an image row v2 about the threshold on which the float evaluation accepts and the all-double one refuses ('f_only') or the reverse
    ('d_only'); None if p1's row has none (the rounding of c decides which of the two exists)"""
    v0 = _v2_for_num(p1[1], F32(np.sqrt(eps) * s), s, cam)
    cand = v0 + (v0 - p1[1]) * 2e-9 * np.arange(-20000, 20001)
    pc = np.stack([np.full(len(cand), 100.0), cand], 1)
    f = epipolar_terms(p1, pc, E, cam)[1] < eps
    d = epipolar_terms(p1, pc, E, cam, all_double=True)[1] < eps
    hit = np.nonzero(f & ~d if kind == "f_only" else d & ~f)[0]
    return cand[hit[len(hit) // 2]] if len(hit) else None


def epipolar_problem(rows, eps, seed, cam=CAM, scale=None):
    """rows[i] = [(distance, kind), ...]: the candidates of row i in frame-2 order, every row in a node of its own, under E = scale * [t]x.
    kind: 'on' the epipolar line (same image row), 'off' (200 rows away), 'under' / 'over' (dsqr = the float just below / just not below
    eps), 'f_only' (the float evaluation accepts, the all-double one does not), 'd_only' (the reverse).  Returns the arrays, E, eps and, per
    frame-2 row, the kind and the float dsqr."""
    rng = np.random.default_rng(seed)
    s, n_under, n_over = threshold_scale(eps)
    if scale is not None:
        s = scale
    E = x_translation(s)
    prob = match_problem([[d for d, _ in r] for r in rows], seed + 1)
    n1, n2 = len(prob["d1"]), len(prob["d2"])
    px1 = np.stack([rng.uniform(20, 300, n1), rng.uniform(40, 200, n1)], 1)
    px2 = np.stack([rng.uniform(20, 300, n2), np.zeros(n2)], 1)
    for i, r in enumerate(rows):                             # a row with a disagreement kind: an image row v1 on which that kind exists
        for kind in [k for _, k in r if k in ("f_only", "d_only")]:
            for _ in range(400):
                if _disagree_v2(px1[i], kind, E, eps, cam, s) is not None:
                    break
                px1[i, 1] = rng.uniform(40, 200)
            else:
                raise AssertionError("no pixel on which the float and the double evaluation disagree (%s)" % kind)
    seen, kinds, dsqr = np.zeros(n1, int), [], np.zeros(n2)
    for j, i in enumerate(prob["owner"]):
        kind = rows[i][seen[i]][1]; seen[i] += 1
        v1 = px1[i, 1]
        if kind == "on":
            v2 = v1
        elif kind == "off":
            v2 = v1 + 200.0
        elif kind in ("under", "over"):
            v2 = _v2_for_num(v1, n_under if kind == "under" else n_over, s, cam)
        else:
            v2 = _disagree_v2(px1[i], kind, E, eps, cam, s)
        px2[j, 1] = v2
        kinds.append(kind)
        dsqr[j] = epipolar_terms(px1[i], px2[j], E, cam)[1][0]
    lo, hi = float_neighbours(eps)
    for j, kind in enumerate(kinds):
        if scale is None:
            assert kind != "under" or dsqr[j] == np.float64(lo), (j, dsqr[j])
            assert kind != "over" or dsqr[j] == np.float64(hi), (j, dsqr[j])
    prob.update(px1=px1, px2=px2, E=E, eps=eps, kinds=kinds, dsqr=dsqr, cam=cam, scale=s)
    return prob


def epipolar_rows(th_low):
    """the mode-1 problem: the replacement rule in both directions (an equal later candidate replaces the earlier one only if it passes the
    epipolar test), th_low - 1, th_low, th_low + 1, and the threshold kinds"""
    T = th_low
    rows = [[(40, "on"), (40, "on")], [(40, "on"), (40, "off")], [(40, "off"), (40, "on")], [(40, "on"), (30, "off"), (35, "on")],
            [(30, "on"), (40, "on")], [(40, "on"), (30, "on")], [(40, "on"), (40, "on"), (40, "on")], [(40, "on"), (40, "under")],
            [(40, "on"), (40, "over")], [(40, "under")], [(40, "over")], [(40, "f_only")], [(40, "d_only")], [(40, "off")], [],
            [(40, "on"), (40, "f_only")], [(40, "on"), (40, "d_only")], [(0, "on")], [(255, "on")], [(0, "on"), (0, "on")]]
    for d in (T - 1, T, T + 1):
        if 0 <= d <= 255:
            rows += [[(d, "on")], [(d, "on"), (d, "on")], [(d, "off"), (d, "on")]]
    if T < 255:
        rows += [[(T, "on"), (T + 1, "on")], [(T + 1, "on"), (T, "on")]]
    return rows


# --------------------------------------------------------------------------------------------------------- related random sets
def related_sets(n1, n2, seed, n_nodes=24, lose=0.1):
    """frame 2 = shuffled, lightly flipped copies of frame 1's rows (cycled or cut to n2 rows); nodes drawn from n_nodes ids, a copy mostly
    keeps its source's node; some nodes are -1 on either side, and some ids occur in one frame only.  Pixels: a copy lies on its source's
    image row, a fraction of a pixel off it, or far off."""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    ids = np.concatenate([np.arange(n_nodes - 2), [NODE_HI, NODE_HI - 1]])
    nd1 = ids[rng.integers(0, len(ids), n1)]
    nd1[rng.random(n1) < lose] = -1
    nd1 = np.where(rng.random(n1) < 0.05, 1000 + rng.integers(0, 3, n1), nd1)                 # ids that frame 2 lacks
    px1 = np.stack([rng.uniform(5, 315, n1), rng.uniform(5, 235, n1)], 1)
    src = rng.permutation(np.resize(np.arange(n1), n2)) if n2 else np.zeros(0, int)
    d2 = d1[src] ^ np.packbits(rng.random((n2, 256)) < 0.04, axis=1)
    nd2 = nd1[src].copy()
    stray = rng.random(n2) < 0.15
    nd2[stray] = ids[rng.integers(0, len(ids), n2)][stray]
    nd2[rng.random(n2) < lose] = -1
    nd2 = np.where(rng.random(n2) < 0.05, 2000 + rng.integers(0, 3, n2), nd2)                 # ids that frame 1 lacks
    off = rng.choice([0.0, 0.0, 0.4, 3.0, 90.0], n2)
    px2 = np.stack([rng.uniform(5, 315, n2), px1[src, 1] + off], 1) if n2 else np.zeros((0, 2))
    return dict(d1=d1, n1=nd1.astype(np.int32), px1=px1, d2=d2, n2=nd2.astype(np.int32), px2=px2)


MATCH_SHAPES = [(1, 0), (1, 1), (63, 255), (64, 256), (65, 257), (255, 513), (256, 768), (257, 1), (513, 768), (513, 0), (256, 255), (257, 513)]


# ------------------------------------------------------------------------------------------------------- orientation problems
def orientation_problem(hist, n1, n2, seed):
    """angles (quarter degrees: exact in float and double) and match12 [n1] whose rotations a1 - a2 fall into the prescribed bins: hist[b]
    matches in bin b (b <= 12: bin = round(rot / 30), Matcher.cpp:251 with the reference's factor), the other rows unmatched, the matched
    rows spread over the whole of match12 (so over every stride of the kernel's 256 lanes)."""
    rng = np.random.default_rng(seed)
    hist = np.asarray(hist, int)
    assert len(hist) == 30 and hist[13:].sum() == 0 and hist.sum() <= n1 and (n2 > 0 or hist.sum() == 0)
    a2 = rng.integers(0, 1440, max(n2, 0)) / 4.0
    a1 = rng.integers(0, 1440, n1) / 4.0
    m = np.full(n1, -1, np.int32)
    rows = rng.permutation(n1)[:hist.sum()]
    bins = rng.permutation(np.repeat(np.arange(30), hist))
    for i, b in zip(rows, bins):
        j = int(rng.integers(0, n2))
        q = int(rng.integers(1, 60) if b == 0 else rng.integers(120 * b - 59, min(120 * b + 60, 1440)))     # rot in quarter degrees
        a1[i] = (a2[j] + q / 4.0) % 360.0
        m[i] = j
    return dict(a1=a1, a2=a2, m=m, hist=hist)


def hist30(**bins):
    h = np.zeros(30, int)
    for b, c in bins.items():
        h[int(b[1:])] = c
    return h


ORIENTATION_HISTS = {
    "three-way tie": hist30(b2=5, b5=5, b7=5),
    "tie of second and third": hist30(b1=9, b4=4, b6=4, b9=2),
    "10 1 1": hist30(b3=10, b0=1, b8=1),
    "10 0 0": hist30(b11=10),
    "100 10 9": hist30(b6=100, b2=10, b12=9),
    "one bin": hist30(b0=37),
    "tie of first and second": hist30(b4=6, b10=6, b1=3),
    "tenth exactly": hist30(b5=20, b6=2, b7=1),
    "all thirteen": np.concatenate([np.arange(13, 0, -1), np.zeros(17, int)]),
}
# angles outside [0, 360) (the reference asserts 0 <= bin < 30): rotations 1000 and -140 fall outside the histogram, 370 and 350 into bin 12
OUTSIDE_ROTATIONS = (np.array([1000.0, 20.0, -500.0, 370.0, -10.0, 2.0]), np.zeros(1), np.zeros(6, np.int32))
EXACT_ROTATIONS = (0.0, 15.0, 45.0, 345.0, float(F32(359.99998)), 14.75, 15.25, 344.75, 29.999998092651367, 180.0)
