"""Lens undistortion on the MI355X (ygz_slam_amd/csrc/undistort.hip: k_undist_map, k_undistort) against the restatement tests/undist_ref.c,
bit for bit: the map of ygz_hip_set_undistortion and level 0 after ygz_hip_build_pyramid_undistorted, for BGR and gray uploads and borders 0
and 200.

Shapes, one small context each: 640 x 480 with 4 slots (16-byte staging loads, dword map loads and stores, 150 tiles per slot); 34 x 32 with
one level, the smallest size ygz_hip_create takes with width % 4 != 0 (byte staging, byte stores, one tile with idle lanes); 202 x 100 with
one level, where a source camera of 4.2 times the focal length makes the whole picture (208 x 100 staged bytes = 20.8 KB) the source box of the
tile around the principal point, beyond the 16 KB a tile stages, so that tile is gathered from global memory with byte stores (the fallback;
at 640 x 480 the four-fold camera takes it in 8 of its 20 tiles that see the picture, with dword stores).  A source camera of
HALF the focal length shrinks the box instead: it is a case of its own.

Then the pipeline behind level 0: levels 1 and 2 are the oracle's pyrDown of it; once one LK call has allocated the tracker's working images
the framed level 0 is its reflect-101 frame; ygz_hip_build_pyramid with a map set is what it is without one; YGZ_E_STATE without a map; the
validation errors through a live context."""
import numpy as np
import pytest

import undist_ref as ur
from conftest import make_ctx

pytestmark = pytest.mark.gpu

SMALL_CAMERA = tuple(float(np.float32(v)) for v in (30.0, 30.5, 17.1, 15.7))
MID_CAMERA = tuple(float(np.float32(v)) for v in (160.0, 160.4, 101.3, 49.7))

# name -> fields of ygz_undistort_params that differ from the defaults (the context's camera, no distortion); f: factor on the source focal length
CASES = {
    "identity": dict(),
    "tum_fr1": dict(ur.TUM_FR1),
    "barrel": dict(k1=-0.4),
    "pincushion": dict(k1=0.3),
    "tangential": dict(p1=0.01, p2=-0.02),
    "half_focal": dict(k1=-0.1, f=0.5),
    "four_times_focal": dict(k1=0.05, f=4.0),
    "zoom_4_2": dict(k1=0.05, f=4.2),
    "nan": dict(k1=1e300),
}


def case_fields(name, cam, border):
    c = dict(CASES[name])
    f = c.pop("f", 1.0)
    return dict(c, fx=cam[0] * f, fy=cam[1] * f, border_value=border)


@pytest.fixture(scope="module")
def vga(hip_lib):
    ctx = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=4)
    yield ctx, ur.DEFAULT_CAMERA
    ctx.close()


@pytest.fixture(scope="module")
def small(hip_lib):
    ctx = make_ctx(hip_lib, width=34, height=32, levels=1, max_frames=2, intrinsics=SMALL_CAMERA)
    yield ctx, SMALL_CAMERA
    ctx.close()


@pytest.fixture(scope="module")
def mid(hip_lib):
    ctx = make_ctx(hip_lib, width=202, height=100, levels=1, max_frames=2, intrinsics=MID_CAMERA)
    yield ctx, MID_CAMERA
    ctx.close()


@pytest.fixture(scope="module")
def pictures():
    return {(w, h): (ur.picture(w, h, 21), ur.picture(w, h, 22, channels=3)) for w, h in ((640, 480), (34, 32), (202, 100))}


def run_case(ctx, cam, name, border, pictures):
    w, h = ctx.width, ctx.height
    gray, bgr = pictures[(w, h)]
    fields = case_fields(name, cam, border)
    p = ctx.set_undistortion(**fields)
    ref = ur.params(cam, **fields)
    assert ur.fields(ref) == {n: getattr(p, n) for n, _ in p._fields_}
    qx, qy = ctx.undistort_map()
    rx, ry = ur.build_map(w, h, ref, cam)
    assert np.array_equal(qx, rx) and np.array_equal(qy, ry), "the map"
    if name == "nan":
        assert (qx == ur.OUTSIDE).all()
    elif name == "identity":
        assert np.array_equal(qx, 32 * np.arange(w)[None, :] + np.zeros((h, 1), np.int64))
    ctx.upload_bgr(0, bgr)
    ctx.upload_gray(1, gray)
    ctx.build_pyramid_undistorted(0, 1, from_bgr=True)
    ctx.build_pyramid_undistorted(1, 1, from_bgr=False)
    assert np.array_equal(ctx.download_level(0, 0), ur.remap(bgr, rx, ry, border)), "level 0 of the BGR upload"
    assert np.array_equal(ctx.download_level(1, 0), ur.remap(gray, rx, ry, border)), "level 0 of the gray upload"
    return qx


@pytest.mark.parametrize("border", [0, 200])
@pytest.mark.parametrize("name", list(CASES))
def test_vga_map_and_image(vga, pictures, name, border):
    ctx, cam = vga
    qx = run_case(ctx, cam, name, border, pictures)
    if name in ("pincushion", "tum_fr1", "four_times_focal"):
        assert (qx == ur.OUTSIDE).any() and (qx != ur.OUTSIDE).any()             # border pixels and partial taps


@pytest.mark.parametrize("border", [0, 200])
@pytest.mark.parametrize("name", list(CASES))
def test_34x32_map_and_image(small, pictures, name, border):
    run_case(*small, name, border, pictures)


@pytest.mark.parametrize("name", ["zoom_4_2", "tum_fr1", "nan"])
def test_202x100_map_and_image(mid, pictures, name):
    run_case(*mid, name, 200, pictures)


def test_three_slots_from_slot_one(vga):
    ctx, cam = vga
    fields = case_fields("tum_fr1", cam, 0)
    ctx.set_undistortion(**fields)
    rx, ry = ur.build_map(640, 480, ur.params(cam, **fields), cam)
    for from_bgr in (True, False):
        imgs = [ur.picture(640, 480, 30 + s, channels=3 if from_bgr else 1) for s in range(4)]
        for s in range(4):
            (ctx.upload_bgr if from_bgr else ctx.upload_gray)(s, imgs[s])
        ctx.build_pyramid(0, 1, from_bgr=from_bgr)
        before = ctx.download_level(0, 0)
        ctx.build_pyramid_undistorted(1, 3, from_bgr=from_bgr)
        for s in range(1, 4):
            assert np.array_equal(ctx.download_level(s, 0), ur.remap(imgs[s], rx, ry, 0)), s
        assert np.array_equal(ctx.download_level(0, 0), before)                   # the slot in front is left alone


def test_the_pipeline_behind_level_zero(vga, oracle, hip_lib):
    ctx, cam = vga
    fields = case_fields("tum_fr1", cam, 0)
    ctx.set_undistortion(**fields)
    p = ur.params(cam, **fields)
    bgr, gray = ur.picture(640, 480, 41, channels=3), ur.picture(640, 480, 42)
    want = [ur.undistort(bgr, p, cam), ur.undistort(gray, p, cam)]
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, 640, 50), rng.uniform(0, 480, 50)], 1).astype(np.float32)

    def build_and_check(framed):
        ctx.upload_bgr(0, bgr)
        ctx.upload_gray(1, gray)
        ctx.build_pyramid_undistorted(0, 1, from_bgr=True)
        ctx.build_pyramid_undistorted(1, 1, from_bgr=False)
        for s in range(2):
            levels = oracle.pyramid(want[s], 3)
            for L in range(3):
                assert np.array_equal(ctx.download_level(s, L), levels[L]), (s, L)
            if framed:
                assert np.array_equal(ctx.download_framed_level(s, 0), np.pad(want[s], 24, mode="reflect")), s
                assert np.array_equal(ctx.download_framed_level(s, 1), np.pad(levels[1], 24, mode="reflect")), s
    build_and_check(False)
    ctx.klt_track(0, 1, pts, pts)                                                 # allocates the tracker's working images
    build_and_check(True)
    # ygz_hip_build_pyramid never undistorts: with a map set it gives what a context without one gives, on every level
    plain = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=2)
    try:
        for c in (ctx, plain):
            c.upload_bgr(0, bgr)
            c.upload_gray(1, gray)
            c.build_pyramid(0, 1, from_bgr=True)
            c.build_pyramid(1, 1, from_bgr=False)
        for s in range(2):
            for L in range(3):
                assert np.array_equal(ctx.download_level(s, L), plain.download_level(s, L)), (s, L)
        assert np.array_equal(plain.download_level(0, 0), ur.gray_of(bgr)) and np.array_equal(plain.download_level(1, 0), gray)
        # no map: the call order is violated; nothing else is
        with pytest.raises(hip_lib.YgzHipError) as e:
            plain.build_pyramid_undistorted(0, 1, from_bgr=True)
        assert e.value.code == hip_lib.E_STATE
        with pytest.raises(hip_lib.YgzHipError) as e:
            plain.undistort_map()
        assert e.value.code == hip_lib.E_STATE
    finally:
        plain.close()
    # a dropped map is no map
    ctx.set_undistortion(drop=True)
    with pytest.raises(hip_lib.YgzHipError) as e:
        ctx.build_pyramid_undistorted(0, 1, from_bgr=True)
    assert e.value.code == hip_lib.E_STATE
    ctx.set_undistortion()
    ctx.build_pyramid_undistorted(0, 1, from_bgr=True)
    assert np.array_equal(ctx.download_level(0, 0), ur.gray_of(bgr))


def test_validation_through_a_live_context(vga, hip_lib):
    ctx, cam = vga
    ctx.set_undistortion()
    d = ctx.default_undistort_params()
    assert (d.k1, d.k2, d.p1, d.p2, d.k3, d.border_value) == (0, 0, 0, 0, 0, 0) and (d.fx, d.fy, d.cx, d.cy) == cam
    for bad in [dict(k1=float("nan")), dict(k2=float("inf")), dict(p1=-float("inf")), dict(p2=float("nan")), dict(k3=float("nan")),
                dict(fx=float("nan")), dict(cy=float("inf")), dict(cx=float("nan")), dict(fx=0.0), dict(fy=-1.0), dict(border_value=-1),
                dict(border_value=256)]:
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.set_undistortion(**bad)
        assert e.value.code == hip_lib.E_INVALID, bad
    # a refused call leaves the map that was set
    qx, _ = ctx.undistort_map()
    assert np.array_equal(qx, 32 * np.arange(640)[None, :] + np.zeros((480, 1), np.int64))
    for slot_begin, n in ((-1, 1), (0, 0), (3, 2), (4, 1)):
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.build_pyramid_undistorted(slot_begin, n, from_bgr=False)
        assert e.value.code == hip_lib.E_INVALID
    lib = hip_lib.load()
    assert lib.ygz_hip_undistort_map(ctx._ctx, None, None) == hip_lib.E_INVALID
    assert lib.ygz_hip_default_undistort_params(ctx._ctx, None) == hip_lib.E_INVALID
