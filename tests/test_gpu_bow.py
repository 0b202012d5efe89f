"""The four kernels of ygz_slam_amd/csrc/bow.hip (k_bow_transform, k_bow_match<0>, k_bow_match<1>, k_bow_orientation) through the C ABI
against the oracle (oracle/bow.c) on the crafted cases of tests/bow_cases.py -- tests/test_bow_cases.py shows on the CPU that each case
tells the rule from its wrong variant.  Every output is an integer or a float weight converted exactly: every comparison is equality.

Which test reaches which rule:
  descent tie (first minimum), node of a shallow leaf (root), parents of 1 / 2 / k children, levelsup 0 .. > L, size_node 48, a second load on a
      live context, the root-only vocabulary                       test_transform_host_form, test_vocabulary_reload_and_root_only
  the slot forms (one launch over several slots / pairs, an empty slot among them)          test_slot_forms
  th_low strict (mode 0), the float ratio product, first of equal bests, best2 = 256, one node per row, a node in one frame only, ids at
      2^31 - 1, the block of 256 rows and the LDS tile of 256 rows    test_search_by_bow_boundaries, test_search_by_bow_shapes
  th_low inclusive (mode 1), last of equal candidates that passes the epipolar test, the float staging at epipolar_dsqr, den < 1e-6, E = 0,
      the context's intrinsics                                        test_triangulation_rules, test_triangulation_den_and_zero, test_triangulation_shapes
  histogram bin = round, the three maxima with ties, the float 0.1 * max1, the stride of 256 rows    test_orientation_host_form
  refusals through a live context                                     test_status_codes"""
import ctypes as C

import numpy as np
import pytest

import bow_cases as bc
import fixtures
from oracle.pyoracle import Camera
from ygz_slam_amd import synth

pytestmark = pytest.mark.gpu
LEVELSUP = (0, 1, 2, 3, 4, 6)
W, H = 320, 240


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=W, height=H, levels=3, max_frames=4, intrinsics=bc.CAM)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cam():
    return Camera(*bc.CAM)


def _same3(got, want, what):
    for g, w, name in zip(got, want, ("word", "weight", "node")):
        assert g.shape == w.shape and np.all(g == w), (what, name, np.nonzero(g != w)[0][:5].tolist())


def _load(ctx, oracle, blob):
    vo = oracle.vocab_parse(blob)
    assert ctx.vocab_load(blob) == (vo.k, vo.L, vo.n_nodes, vo.n_words)
    return vo


# ---------------------------------------------------------------------------------------------------------------- transform
def test_transform_host_form(ctx, oracle):
    blob, meta = bc.ragged_vocabulary(meta=True)
    desc = bc.vocabulary_features(blob, 600, 21)
    per_vocab = {}
    for name, b in (("ragged", blob), ("ragged, size_node 48", bc.ragged_vocabulary(size_node=48)), ("k 3, L 6", fixtures.synthetic_vocabulary(k=3, L=6, seed=9))):
        vo = _load(ctx, oracle, b)
        d = desc if name != "k 3, L 6" else bc.vocabulary_features(b, 600, 22)
        for levelsup in LEVELSUP:
            want = oracle.bow_transform(vo, d, levelsup)[:3]
            for n in (1, 255, 256, 257, 600):                         # the block is 256 lanes
                _same3(ctx.bow_transform(d[:n], levelsup), [w[:n] for w in want], (name, levelsup, n))
            per_vocab[name, levelsup] = want
            if name == "k 3, L 6":
                assert len(np.unique(want[2])) > (1 if levelsup < 6 else 0)
                continue
            word, weight, node = want
            # the forced ties and the shallow leaves were walked (counts from the oracle's own output)
            assert np.isin(word, list(meta["tie_first"])).sum() > 0 and np.isin(word, list(meta["tie_second"])).sum() == 0
            assert all(np.isin(word, meta["shallow"][dep]).sum() > 0 for dep in (1, 2, 3))
            sh = np.isin(word, sum(meta["shallow"].values(), [])) & (weight > 0)
            if levelsup == 0:
                assert sh.sum() > 0 and np.all(node[sh] == 0) and np.all(node[~sh & (weight > 0)] > 0)
            assert (node < 0).sum() == (weight == 0).sum() > 0
    for levelsup in LEVELSUP:                                           # the record size changes nothing
        _same3(per_vocab["ragged", levelsup], per_vocab["ragged, size_node 48", levelsup], levelsup)


def test_vocabulary_reload_and_root_only(ctx, oracle):
    a, b = bc.ragged_vocabulary(), fixtures.synthetic_vocabulary(k=3, L=6, seed=9)
    desc = bc.vocabulary_features(a, 300, 23)
    for blob in (a, b, a):                                             # a second and a third load on the live context
        vo = _load(ctx, oracle, blob)
        for levelsup in (0, 2):
            _same3(ctx.bow_transform(desc, levelsup), oracle.bow_transform(vo, desc, levelsup)[:3], levelsup)
    vo = _load(ctx, oracle, bc.root_only_vocabulary())
    assert (vo.n_nodes, vo.n_words) == (1, 0)
    for levelsup in (0, 4):
        word, weight, node = ctx.bow_transform(desc[:257], levelsup)
        assert np.all(word == -1) and np.all(weight == 0) and np.all(node == -1)
        _same3((word, weight, node), oracle.bow_transform(vo, desc[:257], levelsup)[:3], levelsup)


def _rendered(n):
    tex, m = synth.make_texture(3, W, H, margin=80)
    poses = synth.trajectory(n, 13, 0.3)
    return [synth.render(tex, m, poses[i], W, H, 1.0, 300 + i)[0] for i in range(n)], poses


def test_slot_forms(ctx, oracle, cam):
    """compute_bow / get_bow on three rendered frames and a black one (no keypoints), then both searches and the orientation histogram over
    pairs of slots in one launch, pairs with an empty first or second slot among them"""
    vo = _load(ctx, oracle, bc.ragged_vocabulary())
    imgs, poses = _rendered(3)
    for s in range(3):
        ctx.upload_gray(s, imgs[s])
    ctx.upload_gray(3, np.zeros((H, W), np.uint8))
    ctx.build_pyramid(0, 4); ctx.detect(0, 4)
    kps = [ctx.get_keypoints(s) for s in range(4)]
    assert [len(k["desc"]) > 50 for k in kps] == [True, True, True, False] and len(kps[3]["desc"]) == 0
    K = lambda fx, fy, cx, cy: np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    M = np.linalg.inv(K(synth.FX, synth.FY, synth.CX, synth.CY)) @ K(*bc.CAM)          # the context's normalised coordinates -> the renderer's
    s1, s2 = [1, 2, 0, 3, 0, 2], [0, 1, 0, 0, 3, 0]
    E12 = []
    for a, b in zip(s1, s2):
        T = oracle.se3_mul(poses[min(b, 2)], oracle.se3_inv(poses[min(a, 2)]))           # x2 = R x1 + t; line = pt1^T E12 (Matcher.cpp:341-343)
        R, t = synth.quat_to_R(T[:4]), T[4:]
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        E12.append(M.T @ (tx @ R).T @ M)
    E12 = np.stack(E12)
    total0 = total1 = 0
    for levelsup in (0, 2, 4, 6):
        ctx.compute_bow(0, 4, levelsup)
        nodes = []
        for s in range(4):
            got = ctx.get_bow(s)
            _same3(got, oracle.bow_transform(vo, kps[s]["desc"], levelsup)[:3], (s, levelsup))
            if s < 3:
                _same3(got, ctx.bow_transform(kps[s]["desc"], levelsup), (s, levelsup, "host form"))
            nodes.append(got[2])
        m, cnt = ctx.search_by_bow_slots(s1, s2, mode=0, th_low=65, knn_ratio=0.7)
        mt, ct = ctx.search_by_bow_slots(s1, s2, mode=1, E12=E12, th_low=65, epipolar_dsqr=1e-2)
        kept, hist, ind = ctx.bow_orientation_slots(s1, s2, m)
        for p, (a, b) in enumerate(zip(s1, s2)):
            n1 = len(nodes[a])
            om, oc = oracle.search_by_bow(kps[a]["desc"], nodes[a], kps[b]["desc"], nodes[b], 65, 0.7)
            assert cnt[p] == oc and np.array_equal(m[p, :n1], om[:n1]), (p, levelsup)
            om, oc = oracle.search_for_triangulation(kps[a]["desc"], nodes[a], kps[a]["px"], kps[b]["desc"], nodes[b], kps[b]["px"], E12[p], 65, 1e-2, cam=cam)
            assert ct[p] == oc and np.array_equal(mt[p, :n1], om[:n1]), (p, levelsup)
            oc, oh, oi = oracle.bow_orientation(kps[a]["angle"], kps[b]["angle"] if len(kps[b]["angle"]) else np.zeros(1), m[p, :n1])
            assert kept[p] == oc and np.array_equal(hist[p], oh) and np.array_equal(ind[p], oi), (p, levelsup)
            if 3 in (a, b):
                assert cnt[p] == ct[p] == kept[p] == 0 and list(ind[p]) == [-1, -1, -1]
        assert cnt[2] > 0.8 * (nodes[0] >= 0).sum()                    # a frame against itself
        total0 += int(cnt[:2].sum()); total1 += int(ct[:2].sum())
    assert total0 > 40 and total1 > 20


# ---------------------------------------------------------------------------------------------------- SearchByBoW, mode 0
@pytest.fixture(scope="module")
def boundary():
    return bc.match_problem(bc.boundary_rows(), 31)


def _mode0(ctx, oracle, p, th, ratio, what):
    m, c = ctx.search_by_bow(p["d1"], p["n1"], p["d2"], p["n2"], th_low=th, knn_ratio=ratio)
    om, oc = oracle.search_by_bow(p["d1"], p["n1"], p["d2"], p["n2"], th, ratio)
    assert np.array_equal(m, om), (what, np.nonzero(m != om)[0][:5].tolist())
    assert c == oc == (m >= 0).sum(), what
    return m


@pytest.mark.parametrize("ratio", [0.6, 0.7, 0.8, 0.9, 1.5])
def test_search_by_bow_boundaries(ctx, oracle, boundary, ratio):
    """every row in a node of its own, (best1, best2) prescribed: th_low - 1, th_low, th_low + 1; the float / double triples of the ratio
    sweep (0.6f and 0.8f have them; 0.7f and 0.9f have none, whatever the distances); ties (a ratio above 1 lets them through: the first
    wins); one candidate (best2 = 256); a node that frame 2 lacks; candidates of one row in different LDS tiles"""
    hi = dict(boundary, n1=(bc.NODE_HI - boundary["n1"]).astype(np.int32), n2=(bc.NODE_HI - boundary["n2"]).astype(np.int32))      # ids up to 2^31 - 11
    accepted = 0
    for th in bc.TH_LOWS:
        m = _mode0(ctx, oracle, boundary, th, ratio, (th, ratio))
        assert np.array_equal(_mode0(ctx, oracle, hi, th, ratio, (th, ratio, "high ids")), m)
        accepted += int((m >= 0).sum())
    assert accepted > 100
    if ratio > 1:                                                      # [40, 40, 90]: the first of the two equal bests
        i = boundary["rows"].index([40, 40, 90])
        assert m[i] == np.nonzero(boundary["owner"] == i)[0][0]


@pytest.mark.parametrize("shape", bc.MATCH_SHAPES)
def test_search_by_bow_shapes(ctx, oracle, shape):
    p = bc.related_sets(*shape, seed=100 + shape[0])
    m = _mode0(ctx, oracle, p, 65, 0.7, shape)
    again, _ = ctx.search_by_bow(p["d1"], p["n1"], p["d2"], p["n2"], th_low=65, knn_ratio=0.7)
    assert again.tobytes() == m.tobytes()                              # a second identical call: identical bytes
    if min(shape) >= 63:
        assert (m >= 0).sum() > shape[0] // 8 and np.all(m[p["n1"] < 0] == -1) and not np.isin(m[m >= 0], np.nonzero(p["n2"] < 0)[0]).any()
    one = dict(p, n1=np.full(shape[0], 5, np.int32), n2=np.full(shape[1], 5, np.int32))           # all rows in one node
    _mode0(ctx, oracle, one, 65, 0.7, (shape, "one node"))
    _mode0(ctx, oracle, dict(one, n1=np.full(shape[0], -1, np.int32)), 65, 0.7, (shape, "frame 1 outside the FeatureVector"))
    _mode0(ctx, oracle, dict(one, n2=np.full(shape[1], -1, np.int32)), 65, 0.7, (shape, "frame 2 outside the FeatureVector"))
    _mode0(ctx, oracle, dict(one, n2=np.full(shape[1], 6, np.int32)), 256, 0.9, (shape, "no common node"))


# ------------------------------------------------------------------------------------------- SearchForTriangulation, mode 1
def _mode1(ctx, oracle, cam, p, th, eps, what):
    m, c = ctx.search_by_bow(p["d1"], p["n1"], p["d2"], p["n2"], mode=1, px1=p["px1"], px2=p["px2"], E12=p["E"], th_low=th, epipolar_dsqr=eps)
    om, oc = oracle.search_for_triangulation(p["d1"], p["n1"], p["px1"], p["d2"], p["n2"], p["px2"], p["E"], th, eps, cam=cam)
    assert np.array_equal(m, om), (what, np.nonzero(m != om)[0][:5].tolist())
    assert c == oc == (m >= 0).sum(), what
    return m


@pytest.mark.parametrize("eps", [1e-4, 1e-2])
@pytest.mark.parametrize("th", [0, 1, 50, 65, 256])
def test_triangulation_rules(ctx, oracle, cam, eps, th):
    """the replacement rule in both directions, th_low inclusive, and pixels whose float dsqr is the float just under / just over
    epipolar_dsqr or on which the float and the all-double evaluation disagree; the camera is the context's, not the default"""
    p = bc.epipolar_problem(bc.epipolar_rows(th), eps, 41)
    m = _mode1(ctx, oracle, cam, p, th, eps, (th, eps))
    if th >= 50:
        own = lambda i: list(np.nonzero(p["owner"] == i)[0])
        assert [m[0], m[1], m[2], m[3]] == [own(0)[1], own(1)[0], own(2)[1], own(3)[2]]
        assert [m[7], m[8], m[9], m[10], m[12]] == [own(7)[1], own(8)[0], own(9)[0], -1, -1] and m[11] >= 0
        m_default, _ = oracle.search_for_triangulation(p["d1"], p["n1"], p["px1"], p["d2"], p["n2"], p["px2"], p["E"], th, eps)
        assert not np.array_equal(m_default, m)


def test_triangulation_den_and_zero(ctx, oracle, cam):
    rows = [[(20, "on")], [(20, "on"), (20, "off")], [(20, "off")], [(30, "on"), (20, "on")]] * 70          # 280 rows: two blocks, three tiles
    under, over = bc.den_scales()
    for scale, some in ((under, False), (over, True), (0.0, False), (1.0, True)):
        p = bc.epipolar_problem(rows, 1e-4, 43, scale=scale)
        m = _mode1(ctx, oracle, cam, p, 65, 1e-4, scale)
        assert ((m >= 0).sum() == 210) if some else np.all(m == -1), scale


@pytest.mark.parametrize("shape", bc.MATCH_SHAPES)
def test_triangulation_shapes(ctx, oracle, cam, shape):
    p = dict(bc.related_sets(*shape, seed=200 + shape[0]), E=bc.x_translation())
    for eps in (1e-4, 1e-2):
        m = _mode1(ctx, oracle, cam, p, 65, eps, (shape, eps))
    if min(shape) >= 63:
        assert (m >= 0).sum() > shape[0] // 8
    Rz = np.array([[np.cos(0.3), -np.sin(0.3), 0], [np.sin(0.3), np.cos(0.3), 0], [0, 0, 1]])
    _mode1(ctx, oracle, cam, dict(p, E=bc.x_translation() @ Rz), 256, 1e-2, (shape, "a general E"))
    one = dict(p, n1=np.full(shape[0], 5, np.int32), n2=np.full(shape[1], 5, np.int32))
    _mode1(ctx, oracle, cam, one, 65, 1e-2, (shape, "one node"))


# ---------------------------------------------------------------------------------------------------------- orientation
def _rot(ctx, oracle, a1, a2, m, what):
    got = ctx.bow_orientation(a1, a2, m)
    want = oracle.bow_orientation(a1, a2 if len(a2) else np.zeros(1), m)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (what, got, want)
    return got


def test_orientation_host_form(ctx, oracle):
    want_ind = {"three-way tie": [2, 5, 7], "tie of second and third": [1, 4, 6], "10 1 1": [3, 0, 8], "10 0 0": [11, -1, -1], "100 10 9": [6, 2, -1],
                "one bin": [0, -1, -1], "tie of first and second": [4, 10, 1], "tenth exactly": [5, 6, -1], "all thirteen": [0, 1, 2]}
    for name, hist in bc.ORIENTATION_HISTS.items():
        for n1 in (255, 256, 257, 1000):
            p = bc.orientation_problem(hist, n1, 50, 7 + n1)
            cnt, h, ind = _rot(ctx, oracle, p["a1"], p["a2"], p["m"], (name, n1))
            assert np.array_equal(h, hist) and list(ind) == want_ind[name], (name, n1)
    rots = np.array(bc.EXACT_ROTATIONS)
    for i in range(len(rots)):                                          # n1 = 1
        cnt, h, ind = _rot(ctx, oracle, rots[i:i + 1], np.zeros(1), np.zeros(1, np.int32), rots[i])
        if i < 5:
            assert (cnt, int(np.nonzero(h)[0][0])) == (1, [0, 1, 2, 12, 12][i])                     # 0, 15, 45, 345, 359.99998
    m3 = np.arange(len(rots), dtype=np.int32) % 3
    _rot(ctx, oracle, rots, np.zeros(3), m3, "exact rotations")
    _rot(ctx, oracle, (200.0 + rots) % 360.0, np.full(3, 200.0), m3, "exact rotations across 360")
    assert _rot(ctx, oracle, *bc.OUTSIDE_ROTATIONS, "angles outside [0, 360)")[0] == 4                 # two of the six fall outside the histogram
    for n1, n2 in ((1, 0), (257, 0), (1000, 0), (1000, 5)):            # nothing matched, with and without a second frame
        p = bc.orientation_problem(np.zeros(30, int), n1, n2, 3)
        assert _rot(ctx, oracle, p["a1"], p["a2"], p["m"], (n1, n2))[0] == 0
    for b in (0, 7, 12):                                                # every rotation in one bin, every row matched
        p = bc.orientation_problem(bc.hist30(**{"b%d" % b: 1000}), 1000, 64, 5)
        cnt, h, ind = _rot(ctx, oracle, p["a1"], p["a2"], p["m"], b)
        assert (cnt, h[b], list(ind)) == (1000, 1000, [b, -1, -1])


# --------------------------------------------------------------------------------------------------------- status codes
def test_status_codes(ctx, oracle, cam, hip_lib):
    good = bc.ragged_vocabulary()
    vo = _load(ctx, oracle, good)
    desc = bc.vocabulary_features(good, 100, 24)
    want = oracle.bow_transform(vo, desc, 2)[:3]

    def code(call, *a, **kw):
        with pytest.raises(hip_lib.YgzHipError) as e:
            call(*a, **kw)
        return e.value.code

    for name, bad in bc.invalid_vocabularies().items():
        assert code(ctx.vocab_load, bad) == hip_lib.E_INVALID, name
        _same3(ctx.bow_transform(desc, 2), want, name)                  # the vocabulary loaded before still answers
    assert ctx.lib.ygz_hip_vocab_load(ctx._ctx, None, C.c_size_t(100)) == hip_lib.E_INVALID
    p = bc.related_sets(65, 257, seed=9)
    p["E"] = bc.x_translation()
    args = (p["d1"], p["n1"], p["d2"], p["n2"])
    assert code(ctx.search_by_bow, *args, mode=2) == hip_lib.E_INVALID
    assert code(ctx.search_by_bow, *args, mode=-1) == hip_lib.E_INVALID
    assert code(ctx.search_by_bow, *args, mode=1, px1=p["px1"], px2=p["px2"]) == hip_lib.E_INVALID              # no E12
    assert code(ctx.search_by_bow, *args, mode=1, px2=p["px2"], E12=p["E"]) == hip_lib.E_INVALID                 # no pixels of frame 1
    assert code(ctx.search_by_bow, *args, mode=1, px1=p["px1"], E12=p["E"]) == hip_lib.E_INVALID                 # no pixels of frame 2
    assert code(ctx.search_by_bow_slots, [0], [1], mode=2) == hip_lib.E_INVALID
    assert code(ctx.search_by_bow_slots, [0], [1], mode=1) == hip_lib.E_INVALID                                 # no E12
    assert code(ctx.search_by_bow_slots, [0], [4], mode=0) == hip_lib.E_INVALID                                 # no such slot
    assert code(ctx.bow_transform, desc, -1) == hip_lib.E_INVALID
    o = bc.orientation_problem(bc.ORIENTATION_HISTS["10 1 1"], 257, 50, 1)
    for at in (0, 256):
        m = o["m"].copy(); m[at] = 50                                  # match12[i] >= n2
        assert code(ctx.bow_orientation, o["a1"], o["a2"], m) == hip_lib.E_INVALID
    # a context that never saw a vocabulary
    bare = hip_lib.HipContext(width=W, height=H, levels=3, max_frames=2)
    try:
        assert code(bare.bow_transform, desc, 2) == hip_lib.E_STATE
        assert code(bare.compute_bow, 0, 2, 2) == hip_lib.E_STATE
        assert code(bare.get_bow, 0) == hip_lib.E_STATE
        assert code(bare.search_by_bow_slots, [0], [1], mode=0) == hip_lib.E_STATE
        k = C.c_int(0)
        assert bare.lib.ygz_hip_vocab_info(bare._ctx, C.byref(k), None, None, None) == hip_lib.E_STATE
    finally:
        bare.close()
    # good calls after the refusals
    _same3(ctx.bow_transform(desc, 2), want, "after the refusals")
    _mode0(ctx, oracle, p, 65, 0.7, "after the refusals")
    _mode1(ctx, oracle, cam, p, 65, 1e-4, "after the refusals")
    _rot(ctx, oracle, o["a1"], o["a2"], o["m"], "after the refusals")
