"""Stereo local-map tracking on an indexed map on the MI355X (ygz_hip_stereo_local_map_indexed: k_slm_index in
ygz_slam_amd/csrc/slm_index.hip in front of the five launches of slm.hip) with the rig and the point sets of tests/test_gpu_slm.py.  A map is
the concatenation of several point sets; a frame's set is a list of indices into it.  EVERY output of EVERY frame is bit-identical to
tests/slm_ref.py on the sets gathered by the lists on the host, and, wherever the call by value accepts them (at most 64 lists), to
ygz_hip_stereo_local_map_slots on those gathered sets.  No case is left out of either comparison."""
import numpy as np
import pytest

import slm_ref as sl
from test_gpu_slm import H, K, SHIFT, W, Rig, point_set, same, shifted

pytestmark = pytest.mark.gpu

KEYS = ("pw", "pt_desc", "pt_dmax", "pt_normal")


@pytest.fixture(scope="module")
def rig(hip_lib):
    r = Rig(hip_lib, 3)
    r.sequence()
    r.map, r.home = world(r, (0, 2, 4))
    yield r
    r.ctx.close()


def world(rig, slots):
    """one map: a point set of 700, 400 and 300 points on each of three slots, one behind the other; (map, the first index of each)"""
    parts = [point_set(rig.frames[s], n, 40 + s)[0] for s, n in zip(slots, (700, 400, 300))]
    return {k: np.concatenate([p[k] for p in parts]) for k in KEYS}, np.cumsum([0] + [len(p["pt_dmax"]) for p in parts])


def gathered(pts, idx):
    return {k: pts[k][np.asarray(idx, np.int64)] for k in KEYS} if len(idx) else dict()


def both(rig, pts, lists, slots, li, T, prior=None, stride=None, **kw):
    """the indexed call against the composition and against the call by value on the host-gathered sets"""
    stride = max([len(l) for l in lists] + [1]) if stride is None else stride
    lp = np.full((len(lists), stride), -1, np.int32)                       # the padding is never read: -1 would be refused
    for i, l in enumerate(lists):
        lp[i, :len(l)] = l
    ll = np.array([len(l) for l in lists], np.int32)
    rows = None if prior is None else rig.prior_rows(prior)
    got = rig.ctx.stereo_local_map_indexed(pts, lp, ll, slots, li, T, rows, **kw)
    sets = [gathered(pts, l) for l in lists]
    want = sl.local_map(rig.frames, sets, slots, li, T, prior, cells=rig.ctx.cells, K=K, w=W, h=H, L=rig.levels, **kw)
    same(got, want)
    if len(lists) <= 64:
        same(rig.ctx.stereo_local_map_slots(sets, slots, li, T, rows, **kw), got)
    return got


def priors(rig, rng, lists, slots, li, every=2):
    out = []
    for f, (s, l) in enumerate(zip(slots, li)):
        n_kp, n_pt = len(rig.frames[s]["level"]), len(lists[l])
        p = np.full(n_kp, -1, np.int32)
        if n_pt and f % every == 0:
            who = rng.choice(n_kp, min(n_kp, 30), replace=False)
            p[who] = rng.integers(0, n_pt, len(who))
        out.append(p)
    return out


def edge_lists(rig, rng):
    """lists of 0, 1, 255, 256, 257 and 1025 entries, the long ones on slot 0's part of the map; they overlap, and list 3 names a point twice"""
    a = int(rig.home[1])
    lists = [[], [5], list(range(100, 355)), list(range(200, 456)), list(rng.permutation(a)[:257]), list(rng.permutation(len(rig.map["pt_dmax"]))[:1025])]
    lists[3][10] = lists[3][200]                                           # the same point at two places of one list
    return lists


@pytest.mark.parametrize("with_prior", (False, True))
def test_list_lengths_overlaps_shared_lists_and_slots(rig, with_prior):
    rng = np.random.default_rng(3)
    lists = edge_lists(rig, rng)
    assert [len(l) for l in lists] == [0, 1, 255, 256, 257, 1025] and set(lists[2]) & set(lists[3]) and len(set(lists[3])) == 255
    # frames 2 and 3 share list 2; slot 0 stands under frames 0, 2, 4 and 6 with different poses
    slots, li = [0, 1, 0, 1, 0, 2, 0, 0], [0, 1, 2, 2, 3, 4, 5, 4]
    T = np.stack([shifted(-s * SHIFT + rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)) for s in slots])
    prior = priors(rig, rng, lists, slots, li) if with_prior else None
    got = both(rig, rig.map, lists, slots, li, T, prior, min_edges=1)
    assert got["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(lists[l]) for l in li])]).tolist()
    assert got["counts"][:, 3].tolist() == [len(lists[l]) for l in li] and got["counts"][6, 6] > 50 and (got["status"] == 0).sum() >= 4
    if with_prior:
        assert got["counts"][:, 2].max() > 10


def test_stride_larger_than_every_length(rig):
    rng = np.random.default_rng(4)
    lists = [list(range(0, 300)), list(range(250, 500)), []]
    T = np.stack([shifted(0.3), shifted(-SHIFT), shifted(0.1)])
    a = both(rig, rig.map, lists, [0, 1, 0], [0, 1, 2], T, stride=2048)
    b = both(rig, rig.map, lists, [0, 1, 0], [0, 1, 2], T)
    same(a, b)
    assert a["counts"][0, 6] > 100 and a["status"].tolist()[2] == 1
    # a list nobody reads is neither checked nor gathered
    lp = np.full((2, 8), 10 ** 6, np.int32)
    lp[0, :3] = [1, 2, 3]
    got = rig.ctx.stereo_local_map_indexed(rig.map, lp, [3, 8], [0], [0], [shifted(0.0)])
    assert got["counts"][0, 3] == 3


def test_map_of_one_set_is_the_call_by_value(rig):
    n = int(rig.home[1])
    T = np.stack([shifted(0.4), shifted(-SHIFT + 0.3, 0.2)])
    got = both(rig, rig.map, [list(range(n))], [0, 1], [0, 0], T)
    assert (got["status"] == 0).all() and got["counts"][:, 6].min() > 150


def test_single_level_context(hip_lib):
    r = Rig(hip_lib, 1)
    try:
        for k in range(3):
            r.put(k, k)
        parts = [point_set(r.frames[s], n, 60 + s)[0] for s, n in ((0, 600), (1, 200))]
        pts = {k: np.concatenate([p[k] for p in parts]) for k in KEYS}
        rng = np.random.default_rng(5)
        lists = [list(range(600)), list(rng.permutation(800)[:257]), list(range(590, 800))]
        got = both(r, pts, lists, [0, 1, 2, 1], [0, 1, 0, 2], np.stack([shifted(0.2), shifted(-SHIFT), shifted(-2 * SHIFT), shifted(-SHIFT + 0.2)]))
        assert got["counts"][0, 6] > 100
    finally:
        r.ctx.close()


def test_65_frames_with_65_distinct_lists_on_six_slots(rig, hip_lib):
    rng = np.random.default_rng(6)
    n_map = len(rig.map["pt_dmax"])
    slots = [f % 6 for f in range(65)]
    lists, part = [], [(s // 2) if s % 2 == 0 else int(rng.integers(0, 3)) for s in slots]       # the part of the map a frame looks at
    for f in range(65):
        a, b = int(rig.home[part[f]]), int(rig.home[part[f] + 1])
        lists.append(list(a + rng.permutation(b - a)[:int(rng.integers(40, b - a))]) + list(rng.integers(0, n_map, 7)))
    assert len({tuple(l) for l in lists}) == 65
    li = list(range(65))
    T = np.stack([shifted(-(s - 2 * q) * SHIFT + rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)) for s, q in zip(slots, part)])
    prior = priors(rig, rng, lists, slots, li, every=3)
    # the call by value refuses 65 sets: the composition alone is the reference
    with pytest.raises(hip_lib.YgzHipError) as e:
        rig.ctx.stereo_local_map_slots([gathered(rig.map, l) for l in lists], slots, li, T, rig.prior_rows(prior))
    assert e.value.code == hip_lib.E_CAPACITY
    got = both(rig, rig.map, lists, slots, li, T, prior)
    assert (got["status"] == 0).sum() > 20 and got["counts"][:, 6].sum() > 1000


def test_refusals_through_a_live_context(rig, hip_lib):
    E, ctx, I = hip_lib.YgzHipError, rig.ctx, sl.IDENTITY

    def code(pts, lp, ll, slots, li, T, prior=None, **kw):
        with pytest.raises(E) as e:
            ctx.stereo_local_map_indexed(pts, lp, ll, slots, li, T, prior, **kw)
        return e.value.code
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    lp = np.array([[0, 1, 2, 3]], np.int32)
    assert code(rig.map, lp, [5], [0], [0], [I]) == INV and code(rig.map, lp, [-1], [0], [0], [I]) == INV          # list_len outside [0, stride]
    assert code(rig.map, lp, [4], [0], [1], [I]) == INV and code(rig.map, lp, [4], [0], [-1], [I]) == INV          # the list index
    n_map = len(rig.map["pt_dmax"])
    assert code(rig.map, [[0, n_map, 1, 2]], [4], [0], [0], [I]) == INV and code(rig.map, [[0, -1, 1, 2]], [4], [0], [0], [I]) == INV
    ctx.stereo_local_map_indexed(rig.map, [[0, n_map, 1, 2]], [1], [0], [0], [I])                                   # past list_len: not read
    assert code(dict(), lp, [4], [0], [0], [I]) == INV                                                             # no point to name
    nan = dict(rig.map, pt_normal=rig.map["pt_normal"].copy())
    nan["pt_normal"][n_map - 1, 2] = np.nan                                                                         # a point no list names
    assert code(nan, lp, [4], [0], [0], [I]) == INV
    n = hip_lib.SLM_MAX_FRAMES + 1
    assert code(rig.map, np.zeros((n, 1), np.int32), [1] * n, [0], [0], [I]) == CAP
    assert code(rig.map, lp, [4], [0] * n, [0] * n, np.tile(I, (n, 1)), outputs=False) == CAP
    # the pairs: 1024 frames on a list of 4097 entries; 4096 are the limit itself
    long = np.arange(hip_lib.SLM_MAX_PAIRS // 1024 + 1, dtype=np.int32)[None, :] % n_map
    assert code(rig.map, long, [long.shape[1]], [0] * 1024, [0] * 1024, np.tile(I, (1024, 1)), outputs=False) == CAP
    lim = ctx.stereo_local_map_indexed(rig.map, long, [long.shape[1] - 1], [0] * 1024, [0] * 1024, np.tile(I, (1024, 1)), outputs=False)
    assert (lim["T_out"] == lim["T_out"][0]).all()
    rows = np.full((1, ctx.cells), -1, np.int32)
    rows[0, 3] = 4
    assert code(rig.map, lp, [4], [0], [0], [I], rows) == INV                                                       # a prior past the list
    assert code(rig.map, lp, [4], [9], [0], [I]) == hip_lib.E_STATE and code(rig.map, lp, [4], [10], [0], [I]) == INV
    both(rig, rig.map, [list(range(300))], [0], [0], [shifted(0.2)])                                                # none the worse for it
