"""The restatement of the undistortion stage (tests/undist_ref.c, the frozen spec of DESIGN.md section 18) held to a numpy witness written
another way -- whole-array maps, taps by clipped fancy indexing with an inside mask -- and to what the model must do whatever its code:
identity, a shifted principal point, a half-pixel shift, a round trip through an analytic picture, the border value, coefficients that
overflow, and the rounding tie of rint.  No device."""
import numpy as np
import pytest

import undist_ref as ur

SHAPES = [(640, 480), (1280, 720), (150, 98), (8192, 32)]


def camera_of(w, h):
    """the context's default camera at 640 x 480, else one of the same field of view, as floats converted to double"""
    if (w, h) == (640, 480):
        return ur.DEFAULT_CAMERA
    return tuple(float(np.float32(v)) for v in (0.81 * w, 0.81 * w + 0.1, 0.5 * w + 5.1, 0.5 * h - 0.3))


def witness_map(w, h, p, cam):
    """(mx, my, qx, qy) by whole-array arithmetic in the spec's order"""
    fxd, fyd, cxd, cyd = cam
    u, v = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x, y = (u - cxd) / fxd + 0.0 * v, (v - cyd) / fyd + 0.0 * u
        x2, y2 = x * x, y * y
        r2, xy2 = x2 + y2, 2.0 * (x * y)
        kr = 1.0 + ((p.k3 * r2 + p.k2) * r2 + p.k1) * r2
        xd = (x * kr + p.p1 * xy2) + p.p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p.p1 * (r2 + 2.0 * y2)) + p.p2 * xy2
        mx, my = p.fx * xd + p.cx, p.fy * yd + p.cy
        inside = (mx > -2.0) & (mx < w + 1) & (my > -2.0) & (my < h + 1)
        qx = np.where(inside, np.rint(np.where(inside, mx, 0.0) * 32.0), ur.OUTSIDE).astype(np.int64).astype(np.int32)
        qy = np.where(inside, np.rint(np.where(inside, my, 0.0) * 32.0), ur.OUTSIDE).astype(np.int64).astype(np.int32)
    return mx, my, qx, qy


def witness_remap(gray, qx, qy, border):
    h, w = gray.shape
    valid = qx != ur.OUTSIDE
    q = np.where(valid, qx, 0).astype(np.int64), np.where(valid, qy, 0).astype(np.int64)
    sx, sy = np.floor_divide(q[0], 32), np.floor_divide(q[1], 32)
    ax, ay = q[0] - 32 * sx, q[1] - 32 * sy

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, gray[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), border)
    acc = (32 - ax) * (32 - ay) * tap(sy, sx) + ax * (32 - ay) * tap(sy, sx + 1) + (32 - ax) * ay * tap(sy + 1, sx) + ax * ay * tap(sy + 1, sx + 1)
    return np.where(valid, (acc + 512) >> 10, border).astype(np.uint8)


CASES = {
    "identity": dict(),
    "tum_fr1": dict(ur.TUM_FR1),
    "barrel": dict(k1=-0.4),
    "pincushion": dict(k1=0.3),
    "tangential": dict(p1=0.01, p2=-0.02),
    "mixed": dict(k1=-0.35, k2=0.12, p1=0.001, p2=-0.0007),
    "nan": dict(k1=1e300),
    "inf_minus_inf": dict(k1=1e308, k2=-1e308, k3=1e308),
}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_the_witness(shape):
    w, h = shape
    cam = camera_of(w, h)
    gray, bgr = ur.picture(w, h, 3), ur.picture(w, h, 4, channels=3)
    extras = (dict(), dict(border_value=200), dict(fx=cam[0] / 2, fy=cam[1] / 2), dict(fx=cam[0] * 4, fy=cam[1] * 4, border_value=7))
    if w * h > 640 * 480 or w > 4096:                   # the large shapes: the plain camera and the zoomed one with a border value
        extras = (extras[0], extras[3])
    for name, coeff in CASES.items():
        for extra in extras:
            p = ur.params(cam, **dict(coeff, **extra))
            qx, qy = ur.build_map(w, h, p, cam)
            _, _, wx, wy = witness_map(w, h, p, cam)
            assert np.array_equal(qx, wx) and np.array_equal(qy, wy), (name, extra)
            assert np.array_equal((qx == ur.OUTSIDE), (qy == ur.OUTSIDE))
            assert np.array_equal(ur.remap(gray, qx, qy, p.border_value), witness_remap(gray, qx, qy, p.border_value)), (name, extra)
            # a BGR picture converted per tap equals gray-then-remap
            assert np.array_equal(ur.remap(bgr, qx, qy, p.border_value), witness_remap(ur.gray_of(bgr), qx, qy, p.border_value)), (name, extra)
            if name in ("nan", "inf_minus_inf"):
                assert (qx == ur.OUTSIDE).all() and (ur.remap(gray, qx, qy, p.border_value) == p.border_value).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_identity_shift_and_half_pixel(shape):
    w, h = shape
    cam = camera_of(w, h)
    gray = ur.picture(w, h, 5)
    u = np.arange(w, dtype=np.float64)[None, :]
    # zero coefficients, equal cameras: the picture itself
    p = ur.params(cam)
    mx, my = ur.map_real(w, h, p, cam)
    assert np.abs(mx - u).max() < 1e-12 and np.abs(my - np.arange(h)[:, None]).max() < 1e-12
    assert np.array_equal(ur.undistort(gray, p, cam), gray)
    # the principal point moved by (+3, -2): the picture shifted, the border elsewhere
    for border in (0, 200):
        p = ur.params(cam, cx=cam[2] + 3.0, cy=cam[3] - 2.0, border_value=border)
        want = np.full((h, w), border, np.uint8)
        want[2:, :w - 3] = gray[:h - 2, 3:]
        assert np.array_equal(ur.undistort(gray, p, cam), want)
    # half a pixel to the right: the rounded mean of two neighbours, and half the last column against border 0
    p = ur.params(cam, cx=cam[2] + 0.5)
    g = gray.astype(np.int64)
    want = np.empty((h, w), np.int64)
    want[:, :w - 1] = (g[:, :w - 1] + g[:, 1:] + 1) >> 1
    want[:, w - 1] = (g[:, w - 1] * 512 + 512) >> 10
    assert np.array_equal(ur.undistort(gray, p, cam), want.astype(np.uint8))


def test_the_rounding_tie_goes_to_even():
    # a camera of exactly representable numbers: mx = u + 1/64 and u + 3/64 exactly, so 32 mx = 32 u + 0.5 and 32 u + 1.5
    w, h, cam = 64, 32, (512.0, 512.0, 32.0, 16.0)
    for off, frac in ((1.0 / 64, 0), (3.0 / 64, 2), (5.0 / 64, 2), (7.0 / 64, 4)):
        p = ur.params(cam, cx=cam[2] + off, cy=cam[3] + off)
        mx, _ = ur.map_real(w, h, p, cam)
        assert np.array_equal(mx, np.arange(w)[None, :] + off + np.zeros((h, 1)))
        qx, qy = ur.build_map(w, h, p, cam)
        _, _, wx, wy = witness_map(w, h, p, cam)
        assert np.array_equal(qx, wx) and np.array_equal(qy, wy)
        assert np.array_equal(qx, 32 * np.arange(w)[None, :] + frac + np.zeros((h, 1), np.int64))
        assert np.array_equal(qy, 32 * np.arange(h)[:, None] + frac + np.zeros((1, w), np.int64))
    # the shift is arithmetic: a position left of the picture floors
    p = ur.params(cam, cx=cam[2] - 1.25)
    qx, _ = ur.build_map(w, h, p, cam)
    assert qx[0, 0] == -40 and (qx[0, 0] >> 5, qx[0, 0] & 31) == (-2, 24)


def analytic(x, y):
    return 127.5 + 100.0 * np.sin(2.0 * np.pi * x / 64.0) * np.cos(2.0 * np.pi * y / 48.0)


def undistort_normalised(p, xd, yd, iterations=400):
    """the inverse model by fixed-point iteration: (x, y) with distort(x, y) = (xd, yd), and the residual"""
    x, y = xd.copy(), yd.copy()
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            r2 = x * x + y * y
            kr = 1.0 + ((p.k3 * r2 + p.k2) * r2 + p.k1) * r2
            dx = p.p1 * (2.0 * x * y) + p.p2 * (r2 + 2.0 * x * x)
            dy = p.p1 * (r2 + 2.0 * y * y) + p.p2 * (2.0 * x * y)
            x, y = (xd - dx) / kr, (yd - dy) / kr
        r2 = x * x + y * y
        kr = 1.0 + ((p.k3 * r2 + p.k2) * r2 + p.k1) * r2
        rx = x * kr + p.p1 * (2.0 * x * y) + p.p2 * (r2 + 2.0 * x * x) - xd
        ry = y * kr + p.p1 * (r2 + 2.0 * y * y) + p.p2 * (2.0 * x * y) - yd
    return x, y, np.maximum(np.abs(rx), np.abs(ry))


@pytest.mark.parametrize("name,coeff", [("tum_fr1", ur.TUM_FR1), ("mixed", CASES["mixed"]), ("pincushion", CASES["pincushion"])])
def test_round_trip_through_an_analytic_picture(name, coeff):
    """The analytic picture rendered as the distorted camera sees it, then undistorted: every output pixel whose (mx, my) lies inside the source
    matches the analytic picture at the pixel to < 2 gray levels (0.5 source rounding + 0.5 output rounding + 0.33 bilinear error + 0.36 from
    the 1/32-pixel coordinate grid = 1.69)."""
    w, h, cam = 640, 480, ur.DEFAULT_CAMERA
    p = ur.params(cam, **coeff)
    px, py = np.arange(w, dtype=np.float64)[None, :] + np.zeros((h, 1)), np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    xn, yn, res = undistort_normalised(p, (px - p.cx) / p.fx, (py - p.cy) / p.fy)
    with np.errstate(all="ignore"):
        seen = np.clip(np.rint(analytic(cam[0] * xn + cam[2], cam[1] * yn + cam[3])), 0, 255)
    seen = np.where(np.isfinite(seen), seen, 0).astype(np.uint8)
    out = ur.undistort(seen, p, cam)
    mx, my = ur.map_real(w, h, p, cam)
    inside = (mx >= 0) & (mx <= w - 1) & (my >= 0) & (my <= h - 1)
    assert inside.mean() > 0.5
    # the source pixels those outputs read were rendered from a converged inverse
    used = np.zeros((h, w), bool)
    sx, sy = np.floor(mx[inside]).astype(int), np.floor(my[inside]).astype(int)
    for dy in (0, 1):
        for dx in (0, 1):
            used[np.clip(sy + dy, 0, h - 1), np.clip(sx + dx, 0, w - 1)] = True
    assert res[used].max() <= 1e-15, res[used].max()
    u, v = np.arange(w)[None, :], np.arange(h)[:, None]
    err = np.abs(out.astype(np.float64) - analytic(u + 0.0 * v, v + 0.0 * u))[inside].max()
    print("round trip %s: %.3f gray levels" % (name, err))
    assert err < 2.0, err


def test_distort_point_is_steps_two_and_three():
    p = ur.params(**dict(ur.TUM_FR1, k3=0.0))
    x, y = 0.31, -0.22
    r2 = x * x + y * y
    kr = 1.0 + (p.k2 * r2 + p.k1) * r2
    xd, yd = ur.distort_point(p, x, y)
    assert abs(xd - (x * kr + 2 * p.p1 * x * y + p.p2 * (r2 + 2 * x * x))) < 1e-15
    assert abs(yd - (y * kr + p.p1 * (r2 + 2 * y * y) + 2 * p.p2 * x * y)) < 1e-15
    assert ur.lib().ur_params_size() == 80
