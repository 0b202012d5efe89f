"""The resident map on the MI355X (ygz_slam_amd/csrc/rmap.hip: ygz_hip_map_upload / _update / _download and
ygz_hip_stereo_local_map_resident, k_rmap_filter and k_rmap_scatter around the kernels of lms.hip, mpa.hip, slm_index.hip and slm.hip) with
the rig of tests/test_gpu_slm.py.  A map is made of point sets on the rig's slots, with observations on 3 to 6 keyframes and an attribute row
per observation.  EVERY output of the resident call is compared bit for bit, doubles as their 64 bits, in two ways: with the three existing
device calls (ygz_hip_local_map_select, ygz_hip_map_point_attributes, ygz_hip_stereo_local_map_indexed) joined by the Python filter of
tests/rmap_ref.py, and with tests/rmap_ref.py's composition of the three host references.  No case is left out of either comparison."""
import numpy as np
import pytest

import lms_ref
import rmap_ref as rr
from conftest import make_ctx
from test_gpu_slm import DOUBLES, H, INTS, K, SHIFT, W, Rig, point_set, shifted

pytestmark = pytest.mark.gpu

KEYS = tuple(k for k in DOUBLES + INTS if k != "offsets") + rr.SELECT


@pytest.fixture(scope="module")
def rig(hip_lib):
    r = Rig(hip_lib, 3)
    r.sequence()
    r.world, r.home = world_on(r, ((0, 330), (2, 170), (4, 100)), 5, 11)
    r.rmap = r.ctx.map_create()
    r.rmap.upload(rr.map_arrays(r.world))
    r.resident = r.world
    yield r
    r.ctx.close()


def world_on(rig, parts, n_keyframes, seed):
    """a map of point sets on slots: (world, per point its (slot, keypoint))"""
    sets = [point_set(rig.frames[s], n, seed + s) for s, n in parts]
    pw, desc = np.concatenate([p["pw"] for p, _ in sets]), np.concatenate([p["pt_desc"] for p, _ in sets])
    lv = np.concatenate([rig.frames[s]["level"][j] for (s, _), (_, j) in zip(parts, sets)])
    home = [(s, int(jj)) for (s, _), (_, j) in zip(parts, sets) for jj in j]
    return rr.make_world(pw, desc, lv, n_keyframes, seed), home


def entries(rig, home, slots, seed, frac=0.3, stray=0.0):
    """the points on the frames in keypoint order: keypoint j of a frame on slot s carries, with probability frac, the first point of the
    map made on (s, j), and with probability stray any point"""
    rng = np.random.default_rng(seed)
    first = {}
    for p, h in enumerate(home):
        first.setdefault(h, p)
    off, pt = [0], []
    for s in slots:
        for j in range(len(rig.frames[s]["level"])):
            u = rng.uniform()
            pt.append(first.get((s, j), -1) if u < frac else int(rng.integers(0, len(home))) if u < frac + stray else -1)
        off.append(len(pt))
    return np.array(off, np.int32), np.array(pt, np.int32)


def same(got, want):
    for k in KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), np.ascontiguousarray(w, np.float64).view(np.uint64)
        else:
            assert g.dtype == w.dtype, (k, g.dtype, w.dtype)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)[:6]
            raise AssertionError((k, bad.tolist(), [got[k][tuple(b)] for b in bad], [want[k][tuple(b)] for b in bad]))


def device_composition(rig, world, slots, T, fr_off, fr_pt, lms, **kw):
    """the three existing device calls joined by the Python filter"""
    ctx = rig.ctx
    sel = ctx.local_map_select(world["kf_bad"], world["cov"], world["off"], world["kf"], world["feat"], fr_off, fr_pt, world["pt_bad"], **lms)
    attr = ctx.map_point_attributes(world["center"], world["pw"], world["a_off"], world["a_kf"], world["a_level"])

    def track(points, lists, prior):
        lp = np.full((len(lists), sel["local_pt"].shape[1]), -1, np.int32)
        for f, l in enumerate(lists):
            lp[f, :len(l)] = l
        return ctx.stereo_local_map_indexed(points, lp, [len(l) for l in lists], slots, list(range(len(lists))), T, prior, **kw)
    return rr.join(sel, attr, world, fr_off, ctx.cells, track)


def both(rig, world, slots, T, fr_off, fr_pt, lms=None, rmap=None, **kw):
    """the resident call on `world` (uploaded first when the rig's map holds another) against both compositions"""
    lms = dict(lms or {})
    if rmap is None:
        rmap = rig.rmap
        if rig.resident is not world:
            rmap.upload(rr.map_arrays(world), outputs=False)
            rig.resident = world
    got = rig.ctx.stereo_local_map_resident(rmap, slots, T, fr_off, fr_pt, lms=lms, **kw)
    same(got, rr.resident(world, rig.frames, slots, T, fr_off, fr_pt, rig.ctx.cells, lms, K=K, w=W, h=H, L=rig.levels, **kw))
    same(got, device_composition(rig, world, slots, T, fr_off, fr_pt, lms, **kw))
    return got


def selected(world, fr_off, fr_pt, **lms):
    return lms_ref.select(rr.select_case(world, fr_off, fr_pt, lms))


def poses(slots, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([shifted(-s * SHIFT + rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)) for s in slots])


KINDS = (rr.without_rows, rr.on_centre, rr.no_desc)


@pytest.mark.parametrize("kind", range(3))
def test_refused_point_first_in_the_middle_and_last(rig, kind):
    """a point without attribute rows (state 0), on a centre (state 2) or without a descriptor, at the head, in the middle and at the end"""
    slots = [0]
    fr_off, fr_pt = entries(rig, rig.home, slots, 1)
    sel = selected(rig.world, fr_off, fr_pt)
    n = int(sel["n_pt"][0])
    assert n > 300
    w = rr.copy_world(rig.world)
    at = [0, n // 2, n - 1]
    for i in at:
        KINDS[kind](w, int(sel["local_pt"][0, i]))
    got = both(rig, w, slots, poses(slots), fr_off, fr_pt)
    assert got["n_removed"][0] == 3 and got["n_pt"][0] == n - 3 and got["local_pt"][0, 0] == sel["local_pt"][0, 1]
    assert got["local_pt"][0, n - 4] == sel["local_pt"][0, n - 2] and (got["local_pt"][0, n - 3:] == -1).all()
    assert got["counts"][0, 6] > 50 and got["status"][0] == 0 and got["counts"][0, 2] > 10      # new matches, and a prior that counts


def test_every_point_refused_and_a_frame_without_a_vote(rig):
    slots = [0, 1, 2]
    fr_off, fr_pt = entries(rig, rig.home, slots, 2)
    fr_pt[fr_off[1]:fr_off[2]] = -1                                        # frame 1 votes for nobody
    w = rr.copy_world(rig.world)
    w["pt_has_desc"][:] = 0
    got = both(rig, w, slots, poses(slots), fr_off, fr_pt, min_edges=1)
    assert got["n_pt"].tolist() == [0, 0, 0] and got["n_removed"][0] > 300 and got["n_removed"][1] == 0 and got["n_local"][1] == 0
    assert (got["prior"] == -1).all() and (got["local_pt"] == -1).all() and (got["status"] == 1).all() and (got["match"] == rr.FILL).all()
    # the same frames on the map as it is: frame 1 alone stays empty
    got = both(rig, rig.world, slots, poses(slots), fr_off, fr_pt)
    assert got["n_pt"][1] == 0 and got["ref"][1] == -1 and got["status"][1] == 1 and got["n_pt"][0] > 300 and got["status"][0] == 0


def test_prior_on_a_refused_point_and_a_point_twice_on_a_frame(rig):
    slots = [0]
    fr_off, fr_pt = entries(rig, rig.home, slots, 3)
    on = np.flatnonzero(fr_pt >= 0)
    fr_pt[on[5]] = fr_pt[on[4]]                                            # one point on two keypoints
    sel = selected(rig.world, fr_off, fr_pt)
    assert sel["fr_prior"][on[0]] >= 0 and sel["fr_prior"][on[4]] == sel["fr_prior"][on[5]] >= 0
    w = rr.copy_world(rig.world)
    rr.on_centre(w, int(fr_pt[on[0]]))
    rr.no_desc(w, int(fr_pt[on[1]]))
    got = both(rig, w, slots, poses(slots), fr_off, fr_pt)
    assert got["prior"][0, on[0]] == -1 and got["prior"][0, on[1]] == -1 and got["prior"][0, on[2]] >= 0
    assert got["prior"][0, on[4]] == got["prior"][0, on[5]] >= 0 and got["n_removed"][0] == 2
    assert got["counts"][0, 2] == len(on) - 2


def test_the_cut_stays_out_when_a_kept_point_is_refused(rig):
    slots = [0, 2]
    fr_off, fr_pt = entries(rig, rig.home, slots, 4)
    full = selected(rig.world, fr_off, fr_pt)
    mp = int(full["n_pt"][0]) - 10
    sel = selected(rig.world, fr_off, fr_pt, max_points=mp)
    assert sel["n_cut"][0] == 10 and sel["n_pt"][0] == mp
    w = rr.copy_world(rig.world)
    rr.refuse(w, sel["local_pt"][0, [5, 100, mp - 1]])
    got = both(rig, w, slots, poses(slots), fr_off, fr_pt, lms=dict(max_points=mp))
    assert got["n_cut"][0] == 10 and got["n_removed"][0] == 3 and got["n_pt"][0] == mp - 3
    cut = set(full["local_pt"][0, mp:mp + 10].tolist())
    assert len(cut) == 10 and not cut & set(got["local_pt"][0].tolist())
    assert got["match"].shape == (2, mp) and (got["match"][0, mp - 3:] == rr.FILL).all()


@pytest.fixture(scope="module")
def long_world(rig):
    """600 points that the frame on slot 0 selects in one list"""
    w, home = world_on(rig, ((0, 420), (1, 180)), 3, 21)
    fr_off, fr_pt = entries(rig, home, [0], 5, stray=0.3)
    assert selected(w, fr_off, fr_pt)["n_pt"][0] == 600                    # three keyframes, all of them local
    return w, fr_off, fr_pt


@pytest.mark.parametrize("length", (63, 64, 65, 255, 256, 257, 513))
def test_list_lengths_around_the_wave_and_the_chunk(rig, long_world, length):
    world, fr_off, fr_pt = long_world
    sel = selected(world, fr_off, fr_pt, max_points=length)
    assert sel["n_pt"][0] == length
    w = rr.copy_world(world)
    at = [i for i in (0, 63, 64, 255, 256) if i < length]
    rr.refuse(w, sel["local_pt"][0, at])
    got = both(rig, w, [0], poses([0], length), fr_off, fr_pt, lms=dict(max_points=length))
    assert got["n_removed"][0] == len(at) and got["n_pt"][0] == length - len(at) and got["n_cut"][0] == 600 - length
    keep = np.delete(sel["local_pt"][0, :length], at)
    assert np.array_equal(got["local_pt"][0, :len(keep)], keep)


@pytest.mark.parametrize("slots", ([0], [0, 1, 0, 2, 4]))
def test_one_frame_five_frames_and_two_frames_on_one_slot(rig, slots):
    fr_off, fr_pt = entries(rig, rig.home, slots, 6, stray=0.05)
    w = rr.copy_world(rig.world)
    rr.refuse(w, [3, 50, 51, 52, 331, 400, 599])
    w["kf_bad"][1] = 1
    w["pt_bad"][[10, 11, 340]] = 1
    got = both(rig, w, slots, poses(slots, 7), fr_off, fr_pt, lms=dict(max_keyframes=3), min_edges=1)
    assert (got["n_pt"] > 50).all() and got["counts"][:, 6].sum() > 100 and (got["n_removed"] > 0).all()
    if len(slots) > 1:
        assert not np.array_equal(got["T_out"][0], got["T_out"][2])       # one slot under two poses


def test_update_equals_a_fresh_upload(rig):
    ctx = rig.ctx
    slots = [0, 2]
    fr_off, fr_pt = entries(rig, rig.home, slots, 8)
    a, b = ctx.map_create(), ctx.map_create()
    try:
        a.upload(rr.map_arrays(rig.world))
        w = rr.copy_world(rig.world)
        rng = np.random.default_rng(9)
        pi = rng.choice(600, 70, replace=False).astype(np.int32)
        w["pw"][pi] += rng.uniform(-0.01, 0.01, (70, 3))
        w["pt_desc"][pi[:20], 3] ^= 0x10
        w["pt_bad"][pi[20:25]] = 1
        w["pt_has_desc"][pi[25:30]] = 0
        w["kf_bad"][3] = 1
        w["center"][[0, 4]] += 0.01
        rr.on_centre(w, int(pi[40]))
        a.update(pi, w["pw"][pi], w["pt_desc"][pi], w["pt_bad"][pi], w["pt_has_desc"][pi], [3], [1], [4, 0], w["center"][[4, 0]])
        fresh = b.upload(rr.map_arrays(w))
        da, db = a.download(), b.download()
        for k in da:
            assert da[k].tobytes() == db[k].tobytes(), k
        assert db["state"].tobytes() == fresh["state"].tobytes() and db["dmax"].tobytes() == fresh["dmax"].tobytes()
        assert db["state"][pi[40]] == 2 and a.info()["updates"] == 1 and a.info()["uploads"] == 1
        ga = both(rig, w, slots, poses(slots), fr_off, fr_pt, rmap=a)
        gb = ctx.stereo_local_map_resident(b, slots, poses(slots), fr_off, fr_pt)
        same(ga, gb)
        # a delta of some arrays only, and an empty one
        a.update(pi[:3], pt_bad=[0, 1, 0])
        a.update()
        w["pt_bad"][pi[:3]] = [0, 1, 0]
        b.upload(rr.map_arrays(w), outputs=False)
        da, db = a.download(), b.download()
        assert all(da[k].tobytes() == db[k].tobytes() for k in da) and a.info()["updates"] == 3
    finally:
        a.destroy()
        b.destroy()


def test_smaller_then_larger_two_maps_and_a_repeated_call(rig):
    ctx = rig.ctx
    small, home_s = world_on(rig, ((1, 40),), 3, 31)
    large, home_l = world_on(rig, ((0, 300), (1, 200), (3, 100)), 6, 32)
    a, b = ctx.map_create(), ctx.map_create()
    try:
        info0 = a.info()
        assert info0["n_points"] == 0 and info0["uploads"] == 0
        a.upload(rr.map_arrays(rig.world))
        b.upload(rr.map_arrays(large))
        fo, fp = entries(rig, rig.home, [0, 2], 9)
        first = both(rig, rig.world, [0, 2], poses([0, 2]), fo, fp, rmap=a)
        fl, fpl = entries(rig, home_l, [1, 3], 10)
        both(rig, large, [1, 3], poses([1, 3]), fl, fpl, rmap=b)
        same(ctx.stereo_local_map_resident(a, [0, 2], poses([0, 2]), fo, fp), first)       # b's call did not disturb a, and a repeats itself
        a.upload(rr.map_arrays(small))
        assert a.info()["n_points"] == 40 and a.info()["n_keyframes"] == 3
        fs, fps = entries(rig, home_s, [1], 11, frac=0.5)
        got = both(rig, small, [1], poses([1]), fs, fps, rmap=a)
        assert got["n_pt"][0] == 40 and got["counts"][0, 6] > 5
        a.upload(rr.map_arrays(large))
        both(rig, large, [1, 3], poses([1, 3]), fl, fpl, rmap=a)
        assert a.info()["uploads"] == 3 and a.info()["resident_bytes"] > 0
    finally:
        a.destroy()
        b.destroy()


def test_refusals_leave_the_map_and_the_outputs_alone(rig, hip_lib):
    E, ctx = hip_lib.YgzHipError, rig.ctx
    INV, CAP, STATE = hip_lib.E_INVALID, hip_lib.E_CAPACITY, hip_lib.E_STATE
    m = ctx.map_create()
    slots = [0]
    fr_off, fr_pt = entries(rig, rig.home, slots, 12)
    T = poses(slots)

    def code(fn, *a, **kw):
        with pytest.raises(E) as e:
            fn(*a, **kw)
        return e.value.code
    try:
        # before the first upload
        assert code(m.download) == STATE and code(m.update, [0], pt_bad=[1]) == STATE
        assert code(ctx.stereo_local_map_resident, m, slots, T, fr_off, fr_pt) == STATE
        good = rr.map_arrays(rig.world)
        m.upload(good)
        before = m.download()
        track0 = ctx.stereo_local_map_resident(m, slots, T, fr_off, fr_pt)

        # ---- upload: one hit per check, in the header's order
        def up(**change):
            return code(m.upload, dict(good, **change))
        P = len(rig.world["pw"])
        for name in ("kf_bad", "offsets", "kf", "feat", "cov"):
            assert up(**{name: None}) == INV, name
        assert up(n_keyframes=0) == INV and up(n_points=0) == INV and up(n_cov=-1) == INV
        assert up(n_keyframes=hip_lib.LMS_MAX_KEYFRAMES + 1) == CAP and up(n_cov=hip_lib.LMS_MAX_COV + 1) == CAP
        off = good["offsets"].copy(); off[0] = 1
        assert up(offsets=off) == INV
        off = good["offsets"].copy(); off[5] = off[4] - 1
        assert up(offsets=off) == INV
        kf = good["kf"].copy(); kf[0] = 5
        assert up(kf=kf) == INV
        ft = good["feat"].copy(); ft[3] = hip_lib.LMS_MAX_FEATURES
        assert up(feat=ft) == INV
        cv = good["cov"].copy(); cv[0, 0] = 5
        assert up(cov=cv) == INV
        for name in ("centre", "pw", "a_offsets", "a_kf", "a_level"):
            assert up(**{name: None}) == INV, name
        assert up(n_centres=0) == INV and up(n_centres=hip_lib.MAP_MAX_KEYFRAMES + 1) == CAP
        ao = good["a_offsets"].copy(); ao[0] = 1
        assert up(a_offsets=ao) == INV
        ak = good["a_kf"].copy(); ak[7] = 5
        assert up(a_kf=ak) == INV
        al = good["a_level"].copy(); al[7] = 31
        assert up(a_level=al) == INV
        c = good["centre"].copy(); c[2, 1] = np.inf
        assert up(centre=c) == INV
        x = good["pw"].copy(); x[P - 1, 0] = np.nan
        assert up(pw=x) == INV and up(pt_desc=None) == INV
        second = make_ctx(hip_lib, width=W, height=H, levels=1, max_frames=1)
        try:                                                                # a map of this context through another context
            assert code(Handle(hip_lib, second, m._map).upload, good) == INV and code(Handle(hip_lib, second, m._map).download) == INV
            assert code(second.stereo_local_map_resident, Handle(hip_lib, second, m._map), slots, T, fr_off, fr_pt) == INV
        finally:
            second.close()

        # ---- update
        x3 = np.zeros((2, 3))
        assert code(m.update, [0, P], x3) == INV and code(m.update, [-1, 0], x3) == INV and code(m.update, [4, 4], x3) == INV
        assert code(m.update, [0, 1], [[0, 0, 0], [0, np.nan, 0]]) == INV
        assert code(m.update, kf_idx=[5], kf_bad=[1]) == INV and code(m.update, kf_idx=[1, 1], kf_bad=[1, 1]) == INV
        assert code(m.update, kf_idx=[1]) == INV and code(m.update, c_idx=[1]) == INV
        assert code(m.update, c_idx=[5], centre=[[0, 0, 0]]) == INV and code(m.update, c_idx=[0], centre=[[0, np.inf, 0]]) == INV
        after = m.download()
        assert all(before[k].tobytes() == after[k].tobytes() for k in before)
        assert m.info()["uploads"] == 1 and m.info()["updates"] == 0

        # ---- the tracking call: the outputs keep their pattern
        def track(sl=slots, T_=T, fo=fr_off, fp=fr_pt, rmap=m, **kw):
            c_ = code(ctx.stereo_local_map_resident, rmap, sl, T_, fo, fp, **kw)
            for k, v in ctx.last_outputs.items():
                assert (v == (7 if k == "outlier" else 0 if v.dtype == np.float64 and k != "proj" else -7)).all(), k
            return c_
        n = hip_lib.LMS_MAX_FRAMES + 1
        assert track(sl=[0] * n, T_=np.tile(T, (n, 1)), fo=np.zeros(n + 1, np.int32), fp=[], outputs=False) == CAP
        assert track(lms=dict(max_keyframes=0)) == INV and track(lms=dict(max_points=0)) == INV
        assert track(lms=dict(max_points=hip_lib.SLM_MAX_PAIRS + 1), outputs=False) == CAP
        assert track(fo=[1, fr_off[1]]) == INV and track(sl=[0, 0], T_=np.tile(T, (2, 1)), fo=[0, 5, 4]) == INV
        assert track(fo=[0, hip_lib.LMS_MAX_FEATURES + 1], fp=np.full(hip_lib.LMS_MAX_FEATURES + 1, -1, np.int32)) == CAP
        bad = fr_pt.copy(); bad[2] = P
        assert track(fp=bad) == INV
        bad[2] = -2
        assert track(fp=bad) == INV
        assert track(fo=[0, ctx.cells + 1], fp=np.full(ctx.cells + 1, -1, np.int32)) == INV          # more entries than cells
        assert track(th=0.0) == INV and track(T_=[[0, 0, 0, 1, np.nan, 0, 0]]) == INV
        assert track(sl=[9]) == STATE and track(sl=[10]) == INV
        same(ctx.stereo_local_map_resident(m, slots, T, fr_off, fr_pt), track0)
        handle = m._map
        m.destroy()
        assert code(ctx.stereo_local_map_resident, Handle(hip_lib, ctx, handle), slots, T, fr_off, fr_pt) == INV   # a destroyed map
    finally:
        m.destroy()


def Handle(hip_lib, ctx, handle):
    """a map handle as the bindings pass it, without a live map behind it: a destroyed map, or a map seen through another context"""
    h = hip_lib.ResidentMap.__new__(hip_lib.ResidentMap)
    h.ctx, h.lib, h._map = ctx, ctx.lib, handle
    h.info = lambda: dict(n_keyframes=1, n_points=1, n_centres=1)
    return h
