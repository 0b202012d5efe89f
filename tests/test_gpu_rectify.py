"""Stereo rectification on the MI355X (ygz_slam_amd/csrc/rectify.hip: k_rect_map, k_rect_boxes, k_rectify) against the restatement
tests/rect_ref.c and undist_ref's remap, bit for bit: the maps of ygz_hip_set_rectification and level 0 after
ygz_hip_build_pyramid_rectified.

Shapes, one small context each: 640 x 480 with 6 slots (16-byte staging loads, dword stores; the rig's two cameras on six different
pictures in the orders 010101, 000000, 111111 and 110100 -- the last is out of camera order, so the kernel's walk differs from the slots'
-- for BGR and gray uploads and borders 0 and 200, and from slot 1); 34 x 32 with one level (byte staging, byte stores, one tile with idle
lanes); 202 x 100 (byte stores).  A right camera of 4 and of 4.2 times the focal length makes source boxes beyond the 16 KB a tile stages, so
that tiles are gathered from global memory: the test computes the boxes from the downloaded map and requires both kinds.  A camera turned
by 20 degrees leaves whole tiles outside the picture; a lens with k1 = 1e300 leaves everything outside.

Then the pipeline behind level 0 (the oracle's pyrDown, the tracker's framed copies), one camera with R = I against
ygz_hip_build_pyramid_undistorted (at 640 x 480, and at 34 x 32 and 202 x 100, where both kernels take the byte paths of the body they
share in csrc/remap_dev.h), the other pyramid calls untouched by rig maps, YGZ_E_STATE, the validation errors through a live context,
and the raw textured pair of the rig through upload -> rectify -> detect -> stereo depths against the stereo restatement."""
import ctypes

import numpy as np
import pytest

import rect_ref as rr
import stereo_ref as sr
import undist_ref as ur
from conftest import make_ctx
from test_gpu_undistort import case_fields

pytestmark = pytest.mark.gpu

SMALL_CAMERA = tuple(float(np.float32(v)) for v in (30.0, 30.5, 17.1, 15.7))
MID_CAMERA = tuple(float(np.float32(v)) for v in (160.0, 160.4, 101.3, 49.7))
TILT_20 = rr.rodrigues((0.0, np.deg2rad(20.0), 0.0))


def set_camera(ctx, camera, p):
    """the device's map of rig camera `camera` for the restatement's params p; returns the restatement's map after comparing the two"""
    lens = {n: getattr(p.lens, n) for n, _ in p.lens._fields_}
    got = ctx.set_rectification(camera, R=np.array(list(p.R)), **lens)
    assert bytes(got) == bytes(p)                                                     # the two structs, byte for byte
    return p


def maps_of(ctx, cam, params):
    out = []
    for k, p in enumerate(params):
        set_camera(ctx, k, p)
        qx, qy = ctx.rectify_map(k)
        rx, ry = rr.build_map(ctx.width, ctx.height, p, cam)
        assert np.array_equal(qx, rx) and np.array_equal(qy, ry), "the map of camera %d" % k
        out.append((rx, ry))
    return out


def run(ctx, maps, borders, pattern, imgs, slot_begin=0):
    """imgs: one picture per slot of the call, all BGR or all gray"""
    from_bgr = imgs[0].ndim == 3
    for i, im in enumerate(imgs):
        (ctx.upload_bgr if from_bgr else ctx.upload_gray)(slot_begin + i, im)
    ctx.build_pyramid_rectified(pattern, slot_begin=slot_begin, from_bgr=from_bgr)
    for i, (im, k) in enumerate(zip(imgs, pattern)):
        want = ur.remap(im, maps[k][0], maps[k][1], borders[k])
        got = ctx.download_level(slot_begin + i, 0)
        assert np.array_equal(got, want), "slot %d, camera %d, %s upload" % (slot_begin + i, k, "BGR" if from_bgr else "gray")


@pytest.fixture(scope="module")
def vga(hip_lib):
    ctx = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=6)
    yield ctx, ur.DEFAULT_CAMERA
    ctx.close()


@pytest.fixture(scope="module")
def vga_pictures():
    return ([ur.picture(640, 480, 50 + s) for s in range(6)], [ur.picture(640, 480, 60 + s, channels=3) for s in range(6)])


@pytest.mark.parametrize("border", [0, 200])
def test_vga_rig_patterns(vga, vga_pictures, border):
    ctx, cam = vga
    p0, p1, _ = rr.rig(cam, border)
    p1.lens.border_value = 255 - border                                               # the border value is the camera's own
    maps = maps_of(ctx, cam, (p0, p1))
    borders = (border, 255 - border)
    assert rr.tile_boxes(*maps[0])[..., 4].all() and rr.tile_boxes(*maps[1])[..., 4].all()             # every tile staged
    for pattern in ([0, 1, 0, 1, 0, 1], [0] * 6, [1] * 6, [1, 1, 0, 1, 0, 0]):
        for imgs in vga_pictures:
            run(ctx, maps, borders, pattern, imgs)
    # from slot 1, five slots: the slot in front is left alone
    for imgs in vga_pictures:
        before = ctx.download_level(0, 0)
        run(ctx, maps, borders, [1, 0, 0, 1, 0], imgs[1:], slot_begin=1)
        assert np.array_equal(ctx.download_level(0, 0), before)


def fallback_case(ctx, cam, f, pictures):
    """the rig with the right camera at f times the focal length"""
    p0, p1, _ = rr.rig(cam, 7)
    p1.lens.fx, p1.lens.fy = cam[0] * f, cam[1] * f
    maps = maps_of(ctx, cam, (p0, p1))
    staged = rr.tile_boxes(*maps[1])
    rows = staged[..., 3]
    n_staged, n_fallback = int(((staged[..., 4] == 1) & (rows > 0)).sum()), int(((staged[..., 4] == 0) & (rows > 0)).sum())
    print("right camera at %.1f x the focal length: %d tiles staged, %d gathered" % (f, n_staged, n_fallback))
    assert n_staged >= 1 and n_fallback >= 1
    n = len(pictures[0])
    for imgs in pictures:
        run(ctx, maps, (7, 7), [(i + 1) % 2 for i in range(n)], imgs)


@pytest.mark.parametrize("f", [4.0, 4.2])
def test_vga_boxes_that_do_not_fit(vga, vga_pictures, f):
    ctx, cam = vga
    fallback_case(ctx, cam, f, [p[:2] for p in vga_pictures])


def test_vga_tilt_and_nan(vga, vga_pictures):
    ctx, cam = vga
    p0, p1, _ = rr.rig(cam, 200)
    tilt = rr.params(p0.lens, TILT_20)
    nan = rr.params(ur.params(cam, 200, k1=1e300), np.array(list(p1.R)))
    maps = maps_of(ctx, cam, (tilt, nan))
    box = rr.tile_boxes(*maps[0])
    assert (box[..., 3] == 0).any() and (box[..., 3] > 0).any()                       # whole tiles outside, and tiles that see the picture
    assert (maps[1][0] == rr.OUTSIDE).all()
    for imgs in vga_pictures:
        run(ctx, maps, (200, 200), [0, 1, 0], imgs[:3])
    assert (ctx.download_level(1, 0) == 200).all()


def test_34x32(hip_lib):
    ctx = make_ctx(hip_lib, width=34, height=32, levels=1, max_frames=2, intrinsics=SMALL_CAMERA)
    try:
        pictures = ([ur.picture(34, 32, 70 + s) for s in range(2)], [ur.picture(34, 32, 72 + s, channels=3) for s in range(2)])
        for border in (0, 200):
            p0, p1, _ = rr.rig(SMALL_CAMERA, border)
            maps = maps_of(ctx, SMALL_CAMERA, (p0, p1))
            for pattern in ([0, 1], [1, 0], [1, 1]):
                for imgs in pictures:
                    run(ctx, maps, (border, border), pattern, imgs)
        tilt = rr.params(p0.lens, TILT_20)
        maps = maps_of(ctx, SMALL_CAMERA, (tilt, p1))
        assert (maps[0][0] == rr.OUTSIDE).any()
        for imgs in pictures:
            run(ctx, maps, (200, 200), [0, 1], imgs)
    finally:
        ctx.close()


def test_202x100(hip_lib):
    ctx = make_ctx(hip_lib, width=202, height=100, levels=1, max_frames=2, intrinsics=MID_CAMERA)
    try:
        pictures = ([ur.picture(202, 100, 80 + s) for s in range(2)], [ur.picture(202, 100, 82 + s, channels=3) for s in range(2)])
        p0, p1, _ = rr.rig(MID_CAMERA, 200)
        maps = maps_of(ctx, MID_CAMERA, (p0, p1))
        for imgs in pictures:
            run(ctx, maps, (200, 200), [1, 0], imgs)
        for f in (4.0, 4.2):                                                           # a box beyond 16 KB: gathered, byte stores
            fallback_case(ctx, MID_CAMERA, f, pictures)
    finally:
        ctx.close()


def test_the_pipeline_behind_level_zero(vga, oracle, hip_lib):
    ctx, cam = vga
    p0, p1, _ = rr.rig(cam, 0)
    maps_of(ctx, cam, (p0, p1))
    bgr, gray = ur.picture(640, 480, 41, channels=3), ur.picture(640, 480, 42)
    want = [rr.rectify(bgr, p1, cam), rr.rectify(gray, p0, cam)]
    rng = np.random.default_rng(5)
    pts = np.stack([rng.uniform(0, 640, 50), rng.uniform(0, 480, 50)], 1).astype(np.float32)

    def build_and_check(framed):
        ctx.upload_bgr(0, bgr)
        ctx.upload_gray(1, gray)
        ctx.build_pyramid_rectified([1], slot_begin=0, from_bgr=True)
        ctx.build_pyramid_rectified([0], slot_begin=1, from_bgr=False)
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


def test_one_camera_identity_is_the_lens_only_remap(vga, vga_pictures):
    ctx, cam = vga
    lens = dict(ur.TUM_FR1, border_value=9)
    ctx.set_undistortion(**lens)
    ctx.set_rectification(0, **lens)
    ctx.set_rectification(1, drop=True)
    ux, uy = ctx.undistort_map()
    qx, qy = ctx.rectify_map(0)
    assert np.array_equal(qx, ux) and np.array_equal(qy, uy)
    for imgs in vga_pictures:
        from_bgr = imgs[0].ndim == 3
        for s in range(6):
            (ctx.upload_bgr if from_bgr else ctx.upload_gray)(s, imgs[s])
        ctx.build_pyramid_undistorted(0, 6, from_bgr=from_bgr)
        want = [[ctx.download_level(s, L) for L in range(3)] for s in range(6)]
        for s in range(6):
            (ctx.upload_bgr if from_bgr else ctx.upload_gray)(s, imgs[s])
        ctx.build_pyramid_rectified([0] * 6, from_bgr=from_bgr)
        for s in range(6):
            for L in range(3):
                assert np.array_equal(ctx.download_level(s, L), want[s][L]), (s, L)
    ctx.set_undistortion(drop=True)


@pytest.mark.parametrize("shape", [(34, 32, SMALL_CAMERA), (202, 100, MID_CAMERA)], ids=["34x32", "202x100"])
def test_identity_is_the_lens_only_remap_on_ragged_widths(hip_lib, shape):
    """The same lens through ygz_hip_set_undistortion and through camera 0 of the rig with R = I, at widths that are no multiple of 4 or 16:
    k_undistort and k_rectify go through the byte map loads, the byte staging and the byte stores of the one body they share.  tum_fr1: every
    tile staged; zoom_4_2 at 202 x 100: a tile gathered from global memory."""
    w, h, cam = shape
    ctx = make_ctx(hip_lib, width=w, height=h, levels=1, max_frames=2, intrinsics=cam)
    try:
        gray, bgr = ur.picture(w, h, 90), ur.picture(w, h, 91, channels=3)
        for name in ("tum_fr1", "zoom_4_2"):
            fields = case_fields(name, cam, 200)
            ctx.set_undistortion(**fields)
            ctx.set_rectification(0, **fields)
            rx, ry = ur.build_map(w, h, ur.params(cam, **fields), cam)
            ux, uy = ctx.undistort_map()
            qx, qy = ctx.rectify_map(0)
            assert np.array_equal(ux, rx) and np.array_equal(uy, ry) and np.array_equal(qx, rx) and np.array_equal(qy, ry), name
            box = rr.tile_boxes(rx, ry)
            staged, gathered = (box[..., 4] == 1) & (box[..., 3] > 0), (box[..., 4] == 0) & (box[..., 3] > 0)
            if name == "zoom_4_2" and w == 202:                                        # the whole picture is the box of the tile that sees it
                assert gathered.sum() == 1 and not staged.any()
            else:
                assert staged.any() and not gathered.any(), name
            for im in (bgr, gray):
                from_bgr = im.ndim == 3
                want = ur.remap(im, rx, ry, 200)
                (ctx.upload_bgr if from_bgr else ctx.upload_gray)(0, im)
                ctx.build_pyramid_undistorted(0, 1, from_bgr=from_bgr)
                lens_only = ctx.download_level(0, 0)
                (ctx.upload_bgr if from_bgr else ctx.upload_gray)(1, im)
                ctx.build_pyramid_rectified([0], slot_begin=1, from_bgr=from_bgr)
                rig = ctx.download_level(1, 0)
                assert np.array_equal(lens_only, rig) and np.array_equal(rig, want), (name, "BGR" if from_bgr else "gray")
    finally:
        ctx.close()


def test_the_other_pyramid_calls_do_not_see_the_rig(vga, hip_lib):
    ctx, cam = vga
    p0, p1, _ = rr.rig(cam, 0)
    maps_of(ctx, cam, (p0, p1))
    lens = dict(ur.TUM_FR1)
    ctx.set_undistortion(**lens)
    bgr, gray = ur.picture(640, 480, 43, channels=3), ur.picture(640, 480, 44)
    plain = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=2)
    try:
        plain.set_undistortion(**lens)
        for undistorted in (False, True):
            for c in (ctx, plain):
                c.upload_bgr(0, bgr)
                c.upload_gray(1, gray)
                build = c.build_pyramid_undistorted if undistorted else c.build_pyramid
                build(0, 1, from_bgr=True)
                build(1, 1, from_bgr=False)
            for s in range(2):
                for L in range(3):
                    assert np.array_equal(ctx.download_level(s, L), plain.download_level(s, L)), (undistorted, s, L)
        # no map: the call order is violated; nothing else is
        for call in (lambda: plain.build_pyramid_rectified([0], from_bgr=True), lambda: plain.rectify_map(0), lambda: plain.rectify_map(1)):
            with pytest.raises(hip_lib.YgzHipError) as e:
                call()
            assert e.value.code == hip_lib.E_STATE
        # one camera set: the other is still missing, and a dropped map is no map
        plain.set_rectification(0)
        plain.build_pyramid_rectified([0, 0])
        with pytest.raises(hip_lib.YgzHipError) as e:
            plain.build_pyramid_rectified([0, 1])
        assert e.value.code == hip_lib.E_STATE
        plain.set_rectification(0, drop=True)
        with pytest.raises(hip_lib.YgzHipError) as e:
            plain.build_pyramid_rectified([0])
        assert e.value.code == hip_lib.E_STATE
    finally:
        plain.close()
    ctx.set_undistortion(drop=True)


def test_validation_through_a_live_context(vga, hip_lib):
    ctx, cam = vga
    ctx.set_rectification(0)
    ctx.set_rectification(1)
    d = ctx.default_rectify_params()
    assert (d.lens.k1, d.lens.k2, d.lens.p1, d.lens.p2, d.lens.k3, d.lens.border_value) == (0, 0, 0, 0, 0, 0)
    assert (d.lens.fx, d.lens.fy, d.lens.cx, d.lens.cy) == cam and list(d.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    for bad in [dict(k1=float("nan")), dict(k2=float("inf")), dict(p1=-float("inf")), dict(p2=float("nan")), dict(k3=float("nan")),
                dict(fx=float("nan")), dict(cy=float("inf")), dict(cx=float("nan")), dict(fx=0.0), dict(fy=-1.0), dict(border_value=-1),
                dict(border_value=256), dict(R=np.eye(3) * 1.00001), dict(R=np.diag([1.0, -1.0, 1.0])), dict(R=np.zeros((3, 3))),
                dict(R=np.full((3, 3), np.nan)), dict(R=np.diag([1.0, 1.0, np.inf]))]:
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.set_rectification(0, **bad)
        assert e.value.code == hip_lib.E_INVALID, bad
    for camera in (-1, 2):
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.set_rectification(camera)
        assert e.value.code == hip_lib.E_INVALID
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.rectify_map(camera)
        assert e.value.code == hip_lib.E_INVALID
    # a refused call leaves the map that was set
    qx, _ = ctx.rectify_map(0)
    assert np.array_equal(qx, 32 * np.arange(640)[None, :] + np.zeros((480, 1), np.int64))
    for slot_begin, pattern in ((-1, [0]), (5, [0, 1]), (6, [0]), (0, [0, 2]), (0, [255]), (0, [0] * 7)):
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.build_pyramid_rectified(pattern, slot_begin=slot_begin)
        assert e.value.code == hip_lib.E_INVALID, (slot_begin, pattern)
    lib = hip_lib.load()
    cams = (ctypes.c_uint8 * 2)(0, 1)
    assert lib.ygz_hip_build_pyramid_rectified(ctx._ctx, 0, 0, 0, cams) == hip_lib.E_INVALID
    assert lib.ygz_hip_build_pyramid_rectified(ctx._ctx, 0, 2, 0, None) == hip_lib.E_INVALID
    assert lib.ygz_hip_rectify_map(ctx._ctx, 0, None, None) == hip_lib.E_INVALID
    assert lib.ygz_hip_default_rectify_params(ctx._ctx, None) == hip_lib.E_INVALID


def test_end_to_end_from_the_raw_pair(hip_lib):
    """The raw textured pair of the rig: upload -> ygz_hip_build_pyramid_rectified -> ygz_hip_detect -> ygz_hip_stereo_depths_slots with the
    baseline of ygz_hip_stereo_rectify.  Slots 0, 1: rectified; 2, 3: lens only (R = I); 4, 5: the raw pair as it comes."""
    left, right, _, _ = rr.textured_raw_pair()
    R1, R2, b = hip_lib.stereo_rectify(rr.RIG_R, rr.RIG_T)
    want = rr.stereo_rectify(rr.RIG_R, rr.RIG_T)
    assert np.array_equal(R1, want[0]) and np.array_equal(R2, want[1]) and b == want[2]
    l0, l1 = rr.rig_lenses()
    ctx = make_ctx(hip_lib, width=640, height=480, levels=3, max_frames=6)
    try:
        for s in range(6):
            ctx.upload_gray(s, (left, right)[s % 2])
        maps_of(ctx, ur.DEFAULT_CAMERA, (rr.params(l0, R1), rr.params(l1, R2)))
        ctx.build_pyramid_rectified([0, 1], slot_begin=0)
        maps_of(ctx, ur.DEFAULT_CAMERA, (rr.params(l0), rr.params(l1)))
        ctx.build_pyramid_rectified([0, 1], slot_begin=2)
        ctx.build_pyramid(4, 2)
        ctx.detect(0, 6)
        got = ctx.stereo_depths_slots([0, 2, 4], [1, 3, 5], baseline=b, write_depths=0)
        keys = [k for k in sr.OUTPUTS if k != "counts"]
        share, good = [], []
        for q in range(3):
            a, c = 2 * q, 2 * q + 1
            kl, kr = ctx.get_keypoints(a), ctx.get_keypoints(c)
            levels = [[ctx.download_level(s, L) for L in range(3)] for s in (a, c)]
            ref = sr.match(levels[0], levels[1], sr.keypoints(kl["px"], kl["level"], kl["desc"]), sr.keypoints(kr["px"], kr["level"], kr["desc"]),
                           sr.params(baseline=b))
            n = len(kl["level"])
            for k in keys:
                assert got[k][q, :n].dtype == ref[k].dtype and np.array_equal(got[k][q, :n], ref[k]), (q, k)
            assert np.array_equal(got["counts"][q], ref["counts"])
            ok = got["status"][q, :n] == sr.OK
            share.append(ok.sum() / float(n))
            good.append(float((np.abs(kl["px"][ok, 0] - got["u_right"][q, :n][ok] - rr.RIG_D) < 1.0).mean()) if ok.any() else 0.0)
            if q == 0:
                depth = got["depth"][q, :n][ok]
        print("OK share rectified %.3f, lens only %.3f, raw %.3f; within 1 px of 20: %.3f; median depth %.4f against %.4f"
              % (share[0], share[1], share[2], good[0], np.median(depth), sr.DEFAULT_FX * b / rr.RIG_D))
        assert share[0] >= 0.45 and share[0] >= 3.0 * share[1] and good[0] >= 0.99 and share[1] < 0.2 and share[2] < 0.2
        assert abs(np.median(depth) / (sr.DEFAULT_FX * b / rr.RIG_D) - 1.0) < 0.01
    finally:
        ctx.close()
