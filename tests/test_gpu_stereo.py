"""Stereo input on the MI355X (ygz_slam_amd/csrc/stereo.hip: k_stereo_match, k_stereo_median) against the restatement tests/stereo_ref.c: every
output of every keypoint is EQUAL, doubles included -- right_idx, u_right, depth, sad, status, counts, and the stages best_idx, best_dist,
n_cand, sads.

Shapes, one small context each: 320 x 240 with 3 levels and 4 slots for the scenes a, b, c, e of tests/stereo_ref.py through the array form
(nL = 1, 63, 64, 65 and all 494: the last lane of a wavefront's stride over the right keypoints, one past it, and 8 strides; nR = 0 and nL = 0;
a second parameter set with a disparity window); 34 x 32 with one level, the smallest size ygz_hip_create takes, for the mirror picture with a
keypoint on every column of one row (BORDER on both sides, sr in [10, 23] the only legal strip, the 0.01 branch on the mirror column); 640 x 480
with 3 levels and 8 slots for four pairs of detector keypoints in ONE ygz_hip_stereo_depths_slots call (shift 20, shift 40, identical pictures,
unrelated pictures), which equals four single-pair calls and the restatement on the downloaded keypoints, writes the left slots' depths when
asked and nothing otherwise.  Then every validation error through a live context."""
import numpy as np
import pytest

import stereo_ref as sr
from conftest import make_ctx

pytestmark = pytest.mark.gpu

# a disparity window that cuts into both scenes: in a the fitted disparity of 8 falls below 7.5 for some, in e those of 28 lie at or above 27
WINDOW = dict(min_disparity=7.5, max_disparity=27.0, th_dist=50, baseline=0.537)


def same(got, want, keys):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        bad = np.nonzero(~(got[k] == want[k]).reshape(len(got[k]), -1).all(axis=1))[0] if got[k].ndim else []
        assert np.array_equal(got[k], want[k]), (k, bad[:8], got[k][bad[:8]], want[k][bad[:8]])


@pytest.fixture(scope="module")
def qvga(hip_lib):
    ctx = make_ctx(hip_lib, width=320, height=240, levels=3, max_frames=4)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def loaded(qvga, oracle):
    """name -> the scene, uploaded into slots 0 (left) and 1 (right) the last time it was asked for"""
    state = {"name": None}

    def get(name):
        s = sr.scene(oracle, name)
        if state["name"] != name:
            qvga.upload_gray(0, s.left[0])
            qvga.upload_gray(1, s.right[0])
            qvga.build_pyramid(0, 2)
            for slot, lv in ((0, s.left), (1, s.right)):
                for l in range(3):
                    assert np.array_equal(qvga.download_level(slot, l), lv[l])
            state["name"] = name
        return s
    return get


@pytest.mark.parametrize("n_left", [1, 63, 64, 65, None])
@pytest.mark.parametrize("name", ["a", "b", "c", "e"])
def test_array_form_equals_the_restatement(qvga, loaded, name, n_left):
    s = loaded(name)
    kl = s.kl if n_left is None else sr.head(s.kl, n_left)
    p = sr.params()
    want = sr.match(s.left, s.right, kl, s.kr, p)
    same(qvga.stereo_match(0, 1, kl, s.kr, **sr.fields(p)), want, sr.OUTPUTS)
    same(qvga.stereo_candidates(0, 1, kl, s.kr, **sr.fields(p)), want, sr.STAGES)
    if n_left is None:
        assert want["counts"][sr.OK] > 100                                        # the case is about something


@pytest.mark.parametrize("name", ["a", "e"])
def test_disparity_window_and_threshold(qvga, loaded, name):
    s = loaded(name)
    p = sr.params(**WINDOW)
    want = sr.match(s.left, s.right, s.kl, s.kr, p)
    assert want["counts"][sr.DISPARITY] > 10 and want["counts"][sr.OK if name == "a" else sr.NO_CANDIDATE] > 30           # the case is about something
    same(qvga.stereo_match(0, 1, s.kl, s.kr, **sr.fields(p)), want, sr.OUTPUTS)
    same(qvga.stereo_candidates(0, 1, s.kl, s.kr, **sr.fields(p)), want, sr.STAGES)
    # the slots the other way round: other pictures behind the same keypoints
    want = sr.match(s.right, s.left, s.kl, s.kr, p)
    same(qvga.stereo_match(1, 0, s.kl, s.kr, **sr.fields(p)), want, sr.OUTPUTS)


def test_empty_lists(qvga, loaded):
    s = loaded("a")
    none = sr.head(s.kr, 0)
    got = qvga.stereo_match(0, 1, s.kl, none)
    same(got, sr.match(s.left, s.right, s.kl, none, sr.params()), sr.OUTPUTS)
    assert (got["status"] == sr.NO_CANDIDATE).all() and got["counts"][sr.NO_CANDIDATE] == len(s.kl["level"])
    got = qvga.stereo_candidates(0, 1, s.kl, none)
    assert (got["best_idx"] == -1).all() and (got["best_dist"] == -1).all() and (got["n_cand"] == 0).all() and (got["sads"] == -1).all()
    got = qvga.stereo_match(0, 1, sr.head(s.kl, 0), s.kr)
    assert len(got["status"]) == 0 and not got["counts"].any()
    assert len(qvga.stereo_candidates(0, 1, sr.head(s.kl, 0), s.kr)["n_cand"]) == 0


def test_smallest_context_mirror_picture(hip_lib, oracle):
    s = sr.scene(oracle, "d")
    fx = float(np.float32(30.0))
    # a cell of 4 pixels: 9 x 8 = 72 cells, so that the 34 keypoints of the row fit ygz_hip_max_keypoints
    ctx = make_ctx(hip_lib, width=34, height=32, levels=1, max_frames=2, cell_size=4, intrinsics=(30.0, 30.5, 17.1, 15.7))
    try:
        ctx.upload_gray(0, s.left[0])
        ctx.upload_gray(1, s.right[0])
        ctx.build_pyramid(0, 2)
        assert ctx.cells == 72
        p = sr.params(baseline=0.25)
        want = sr.match(s.left, s.right, s.kl, s.kr, p, fx=fx)
        got = ctx.stereo_match(0, 1, s.kl, s.kr, **sr.fields(p))
        same(got, want, sr.OUTPUTS)
        same(ctx.stereo_candidates(0, 1, s.kl, s.kr, **sr.fields(p)), want, sr.STAGES)
        st = got["status"]
        assert (st[:10] == sr.BORDER).all() and (st[24:] == sr.BORDER).all() and (st[10:24] != sr.BORDER).all()
        assert st[16] == sr.OK and got["u_right"][16] == 16.0 - 0.01 and got["depth"][16] == fx * 0.25 / 0.01          # disparity 0: the 0.01 branch
    finally:
        ctx.close()


# ---- the slot form: four pairs of detector keypoints in one call ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vga(hip_lib, oracle):
    ctx = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=8)
    pairs = [sr.detector_pair(oracle, 640, 480, 20, 31), sr.detector_pair(oracle, 640, 480, 40, 32), sr.detector_pair(oracle, 640, 480, 0, 33),
             sr.detector_pair(oracle, 640, 480, 0, 34, other_seed=35)]
    imgs = np.ascontiguousarray(np.stack([im for pr in pairs for im in pr]))          # slots 0, 2, 4, 6 left; 1, 3, 5, 7 right
    ctx.upload_gray_batch(0, imgs)
    ctx.build_pyramid(0, 8)
    ctx.detect(0, 8)
    kps = [ctx.get_keypoints(s) for s in range(8)]
    levels = [[ctx.download_level(s, l) for l in range(3)] for s in range(8)]
    yield ctx, kps, levels
    ctx.close()


LEFT, RIGHT = [0, 2, 4, 6], [1, 3, 5, 7]


@pytest.fixture(scope="module")
def vga_reference(vga):
    _, kps, levels = vga
    return [sr.match(levels[a], levels[b], sr.keypoints(kps[a]["px"], kps[a]["level"], kps[a]["desc"]),
                     sr.keypoints(kps[b]["px"], kps[b]["level"], kps[b]["desc"]), sr.params()) for a, b in zip(LEFT, RIGHT)]


def test_batched_slot_form(vga, vga_reference):
    ctx, kps, _ = vga
    keys = [k for k in sr.OUTPUTS if k != "counts"]
    got = ctx.stereo_depths_slots(LEFT, RIGHT, write_depths=0)
    for q, (a, b) in enumerate(zip(LEFT, RIGHT)):
        n, want = len(kps[a]["level"]), vga_reference[q]
        assert n > 1000
        same({k: got[k][q, :n] for k in keys}, want, keys)
        assert np.array_equal(got["counts"][q], want["counts"]) and got["counts"][q].sum() == n
        for k in keys:
            assert (got[k][q, n:] == -1).all(), k
        one = ctx.stereo_depths_slots([a], [b], write_depths=0)
        for k in sr.OUTPUTS:
            assert np.array_equal(one[k][0], got[k][q]), (q, k)
        # the array form on the downloaded keypoints is the same computation
        arr = ctx.stereo_match(a, b, kps[a], kps[b])
        same(arr, want, sr.OUTPUTS)
    c = got["counts"]
    # shift 20: nearly every keypoint away from the borders is found; unrelated pictures: hardly any
    assert c[0][sr.OK] > 0.6 * c[0].sum() and c[1][sr.OK] > 0.2 * c[1].sum() and c[3][sr.OK] < 0.05 * c[3].sum()
    px, lv, st = kps[0]["px"], kps[0]["level"], got["status"][0, :len(kps[0]["level"])]
    m = 24.0 * np.exp2(lv)
    inner = (px[:, 0] - 20 >= m) & (px[:, 0] < 640 - m) & (px[:, 1] >= m) & (px[:, 1] < 480 - m)
    print("shift 20: %d of %d keypoints 24 * 2^l from the borders OK; counts per pair %s" % ((st[inner] == sr.OK).sum(), inner.sum(), c.tolist()))


def test_write_depths(vga, vga_reference):
    ctx, kps, _ = vga
    for s in range(8):
        n = len(kps[s]["level"])
        ctx.set_keypoint_depths(s, np.full(n, 7.0 + s), np.full(n, s % 2, np.uint8))
    before = [ctx.get_keypoint_depths(s) for s in range(8)]
    ctx.stereo_depths_slots(LEFT, RIGHT, write_depths=0)
    for s in range(8):
        d, m = ctx.get_keypoint_depths(s)
        assert np.array_equal(d, before[s][0]) and np.array_equal(m, before[s][1]), s
    got = ctx.stereo_depths_slots(LEFT, RIGHT)                                      # write_depths = 1 is the default
    for q, (a, b) in enumerate(zip(LEFT, RIGHT)):
        d, m = ctx.get_keypoint_depths(a)
        want = vga_reference[q]
        assert np.array_equal(d, want["depth"]) and np.array_equal(m, (want["status"] == sr.OK).astype(np.uint8)), q
        assert np.array_equal(got["depth"][q, :len(d)], d)
        d, m = ctx.get_keypoint_depths(b)
        assert np.array_equal(d, before[b][0]) and np.array_equal(m, before[b][1]), b
    assert hip_default(ctx).write_depths == 1


def hip_default(ctx):
    return ctx.default_stereo_params()


def test_defaults(vga):
    p = hip_default(vga[0])
    assert (p.baseline, p.min_disparity, p.max_disparity, p.th_dist, p.write_depths) == (0.1, 0.0, 0.0, 75, 1)


def test_validation_errors(vga, hip_lib):
    ctx, kps, _ = vga
    lib = hip_lib.load()
    hip_lib.stereo_argtypes(lib)
    INV, CAP, STATE = hip_lib.E_INVALID, hip_lib.E_CAPACITY, hip_lib.E_STATE
    kl, kr = kps[0], kps[1]

    def code(f, *a, **kw):
        with pytest.raises(hip_lib.YgzHipError) as e:
            f(*a, **kw)
        return e.value.code
    bad_params = [dict(baseline=0.0), dict(baseline=-0.1), dict(baseline=float("nan")), dict(baseline=float("inf")), dict(min_disparity=-1.0),
                  dict(min_disparity=float("nan")), dict(max_disparity=-1.0), dict(max_disparity=float("inf")), dict(th_dist=-1), dict(th_dist=257)]
    for bad in bad_params:
        assert code(ctx.stereo_depths_slots, [0], [1], **bad) == INV, bad
        assert code(ctx.stereo_match, 0, 1, kl, kr, **bad) == INV, bad
        assert code(ctx.stereo_candidates, 0, 1, kl, kr, **bad) == INV, bad
    for th in (0, 256):
        ctx.stereo_match(0, 1, sr.head(kl, 3), kr, th_dist=th)
    for ls, rs in (([-1], [1]), ([8], [1]), ([0], [-1]), ([0], [8]), ([2], [2]), ([0, 0], [1, 3]), ([], [])):
        assert code(ctx.stereo_depths_slots, ls, rs, write_depths=0) == INV, (ls, rs)
    ctx.stereo_depths_slots([0, 2], [1, 1], write_depths=0)                        # one right picture for two left ones is legal
    for a, b in ((-1, 1), (8, 1), (0, -1), (0, 8), (3, 3)):
        assert code(ctx.stereo_match, a, b, kl, kr) == INV and code(ctx.stereo_candidates, a, b, kl, kr) == INV, (a, b)
    for side in (0, 1):
        for lvl in (-1, 3):
            k = sr.head(kps[side], 5)
            k["level"][4] = lvl
            args = (k, kr) if side == 0 else (sr.head(kl, 5), k)
            assert code(ctx.stereo_match, 0, 1, *args) == INV and code(ctx.stereo_candidates, 0, 1, *args) == INV, (side, lvl)
    # null pointers
    p = ctx.default_stereo_params()
    import ctypes as C
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    one, two = np.array([0], np.int32), np.array([1], np.int32)
    assert lib.ygz_hip_stereo_depths_slots(ctx._ctx, 1, ip(one), ip(two), None, None, None, None, None, None, None) == INV
    assert lib.ygz_hip_stereo_depths_slots(ctx._ctx, 1, None, ip(two), C.byref(p), None, None, None, None, None, None) == INV
    assert lib.ygz_hip_stereo_depths_slots(ctx._ctx, 1, ip(one), None, C.byref(p), None, None, None, None, None, None) == INV
    assert lib.ygz_hip_stereo_depths_slots(ctx._ctx, 0, ip(one), ip(two), C.byref(p), None, None, None, None, None, None) == INV
    assert lib.ygz_hip_stereo_depths_slots(None, 1, ip(one), ip(two), C.byref(p), None, None, None, None, None, None) == INV
    p.write_depths = 0
    assert lib.ygz_hip_stereo_depths_slots(ctx._ctx, 1, ip(one), ip(two), C.byref(p), None, None, None, None, None, None) == hip_lib.OK   # every output may be NULL
    dp, bp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
    L3 = (dp(kl["px"]), ip(kl["level"]), bp(kl["desc"]), 3)
    R3 = (dp(kr["px"]), ip(kr["level"]), bp(kr["desc"]), 3)
    tail6, tail4 = (None,) * 6, (None,) * 4
    assert lib.ygz_hip_stereo_match(ctx._ctx, 0, 1, *L3, *R3, C.byref(p), *tail6) == hip_lib.OK
    assert lib.ygz_hip_stereo_match(ctx._ctx, 0, 1, *L3, *R3, None, *tail6) == INV
    assert lib.ygz_hip_stereo_match(None, 0, 1, *L3, *R3, C.byref(p), *tail6) == INV
    for k in range(3):
        broken = list(L3)
        broken[k] = None
        assert lib.ygz_hip_stereo_match(ctx._ctx, 0, 1, *broken, *R3, C.byref(p), *tail6) == INV
        assert lib.ygz_hip_stereo_match(ctx._ctx, 0, 1, *L3, *broken, C.byref(p), *tail6) == INV
        assert lib.ygz_hip_stereo_candidates(ctx._ctx, 0, 1, *broken, *R3, C.byref(p), *tail4) == INV
    assert lib.ygz_hip_stereo_match(ctx._ctx, 0, 1, L3[0], L3[1], L3[2], -1, *R3, C.byref(p), *tail6) == INV
    # capacity: more keypoints than ygz_hip_max_keypoints
    big = ctx.cells + 1
    many = sr.keypoints(np.zeros((big, 2)), np.zeros(big, np.int32), np.zeros((big, 32), np.uint8))
    assert code(ctx.stereo_match, 0, 1, many, kr) == CAP and code(ctx.stereo_match, 0, 1, kl, many) == CAP
    assert code(ctx.stereo_candidates, 0, 1, many, kr) == CAP


def test_state_errors(hip_lib, oracle):
    ctx = make_ctx(hip_lib, width=320, height=240, levels=3, max_frames=4)
    try:
        s = sr.scene(oracle, "a")
        few = sr.head(s.kl, 4)

        def code(f, *a, **kw):
            with pytest.raises(hip_lib.YgzHipError) as e:
                f(*a, **kw)
            return e.value.code
        assert code(ctx.stereo_match, 0, 1, few, few) == hip_lib.E_STATE                     # no pyramid in either slot
        ctx.upload_gray(0, s.left[0])
        ctx.build_pyramid(0, 1)
        assert code(ctx.stereo_match, 0, 1, few, few) == hip_lib.E_STATE and code(ctx.stereo_candidates, 1, 0, few, few) == hip_lib.E_STATE
        ctx.upload_gray(1, s.right[0])
        ctx.build_pyramid(1, 1)
        ctx.stereo_match(0, 1, few, few)
        assert code(ctx.stereo_depths_slots, [0], [1]) == hip_lib.E_STATE                    # pyramids, but no keypoints
        ctx.detect(0, 1)
        assert code(ctx.stereo_depths_slots, [0], [1]) == hip_lib.E_STATE
        ctx.detect(1, 1)
        ctx.stereo_depths_slots([0], [1])
        ctx.upload_gray(1, s.right[0])                                                       # a new upload: the slot's pyramid is gone
        assert code(ctx.stereo_depths_slots, [0], [1]) == hip_lib.E_STATE
    finally:
        ctx.close()
