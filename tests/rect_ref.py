"""ctypes loader of tests/rect_ref.c, the restatement of the stereo rectification (ygz_slam_amd/csrc/rectify.hip) that tests/test_rect_ref.py
holds to a numpy witness and tests/test_gpu_rectify.py holds the device against.  The remap behind the map is undist_ref's (ur.remap).  Test
infrastructure: compiled with gcc into a temporary directory the first time it is used, never imported by the package.  Also the rig and the
pictures the tests share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import undist_ref as ur

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

OUTSIDE = ur.OUTSIDE
IDENTITY = np.eye(3)


class Params(ctypes.Structure):
    """rr_params = ygz_rectify_params"""
    _fields_ = [("lens", ur.Params), ("R", ctypes.c_double * 9)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="rect_ref_")
        so = os.path.join(d, "librect_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "rect_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        dbl, dp, ip = ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        _lib.rr_stereo_rectify.argtypes = [dp, dp, dp, dp, dp]
        _lib.rr_rotation_check.argtypes = [dp]
        _lib.rr_map.argtypes = [ctypes.c_int, ctypes.c_int, dbl, dbl, dbl, dbl, ctypes.POINTER(Params), ip, ip]
        _lib.rr_map_real.argtypes = [ctypes.c_int, ctypes.c_int, dbl, dbl, dbl, dbl, ctypes.POINTER(Params), dp, dp, ctypes.POINTER(ctypes.c_uint8)]
        _lib.rr_map.restype = _lib.rr_map_real.restype = None
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(lens, R=IDENTITY):
    """lens: an ur.Params; R: [3, 3] (R1 or R2)"""
    return Params(lens, (ctypes.c_double * 9)(*[float(v) for v in np.asarray(R, np.float64).reshape(9)]))


def stereo_rectify(R, T):
    """rr_stereo_rectify: (R1, R2, baseline), or None when the rig is refused"""
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    T = np.ascontiguousarray(T, np.float64).reshape(3)
    R1, R2, b = np.zeros(9), np.zeros(9), ctypes.c_double(0)
    rc = lib().rr_stereo_rectify(_p(R, ctypes.c_double), _p(T, ctypes.c_double), _p(R1, ctypes.c_double), _p(R2, ctypes.c_double), ctypes.byref(b))
    return None if rc else (R1.reshape(3, 3), R2.reshape(3, 3), b.value)


def build_map(w, h, p, camera=ur.DEFAULT_CAMERA):
    """rr_map: (qx, qy) [h, w] int32 for the output camera `camera`"""
    qx, qy = np.empty((h, w), np.int32), np.empty((h, w), np.int32)
    lib().rr_map(w, h, *[float(c) for c in camera], ctypes.byref(p), _p(qx, ctypes.c_int32), _p(qy, ctypes.c_int32))
    return qx, qy


def map_real(w, h, p, camera=ur.DEFAULT_CAMERA):
    """(mx, my, front): the source pixel of every output pixel and whether it lies in front of the source camera"""
    mx, my, front = np.empty((h, w), np.float64), np.empty((h, w), np.float64), np.empty((h, w), np.uint8)
    lib().rr_map_real(w, h, *[float(c) for c in camera], ctypes.byref(p), _p(mx, ctypes.c_double), _p(my, ctypes.c_double), _p(front, ctypes.c_uint8))
    return mx, my, front.astype(bool)


def rectify(src, p, camera=ur.DEFAULT_CAMERA):
    h, w = src.shape[:2]
    qx, qy = build_map(w, h, p, camera)
    return ur.remap(src, qx, qy, p.lens.border_value)


def rodrigues(om):
    """the rotation matrix of a rotation vector, as OpenCV orders it: cos I + (1 - cos) r r^T + sin [r]x"""
    om = np.asarray(om, np.float64)
    th = float(np.sqrt(om @ om))
    if th < 2.220446049250313e-16:
        return np.eye(3)
    r = om / th
    K = np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])
    return np.cos(th) * np.eye(3) + (1.0 - np.cos(th)) * np.outer(r, r) + np.sin(th) * K


# ---- the rig of the tests: VGA, EuRoC-like lenses, a relative rotation of about 1.5 degrees, a baseline of 11 cm not exactly along x
RIG_W, RIG_H, RIG_D = 640, 480, 20
RIG_R = rodrigues((0.010, -0.020, 0.015))
RIG_T = np.array([-0.11, 0.002, -0.003])


def rig_lenses(camera=ur.DEFAULT_CAMERA, border_value=0):
    fx, fy, cx, cy = camera
    left = ur.params(camera, border_value, k1=-0.2834, k2=0.0740, p1=0.00019, p2=0.0000176, fx=0.98 * fx, fy=0.985 * fy, cx=cx + 6.0, cy=cy - 4.0)
    right = ur.params(camera, border_value, k1=-0.2837, k2=0.0745, p1=-0.00010, p2=-0.0000356, fx=0.975 * fx, fy=0.98 * fy, cx=cx - 5.0, cy=cy + 7.0)
    return left, right


def rig(camera=ur.DEFAULT_CAMERA, border_value=0):
    """(params of camera 0, params of camera 1, baseline)"""
    R1, R2, b = stereo_rectify(RIG_R, RIG_T)
    left, right = rig_lenses(camera, border_value)
    return params(left, R1), params(right, R2), b


def raw_positions(p, w, h, camera=ur.DEFAULT_CAMERA):
    """where every raw pixel of camera p looks in the ideal (rectified) picture: the lens inverted by fixed-point iteration, the ray turned by
    Rk, projected with `camera`.  (x, y, residual of the inversion)"""
    from test_undist_ref import undistort_normalised
    l = p.lens
    R = np.array(list(p.R)).reshape(3, 3)
    px, py = np.arange(w, dtype=np.float64)[None, :] + np.zeros((h, 1)), np.arange(h, dtype=np.float64)[:, None] + np.zeros((1, w))
    xn, yn, res = undistort_normalised(l, (px - l.cx) / l.fx, (py - l.cy) / l.fy)
    with np.errstate(all="ignore"):
        X = R[0, 0] * xn + R[0, 1] * yn + R[0, 2]
        Y = R[1, 0] * xn + R[1, 1] * yn + R[1, 2]
        W = R[2, 0] * xn + R[2, 1] * yn + R[2, 2]
        return camera[0] * (X / W) + camera[2], camera[1] * (Y / W) + camera[3], res


def render_analytic(p, f, w, h, camera=ur.DEFAULT_CAMERA):
    """the raw picture of camera p of the ideal picture f(x, y), exact up to the rounding to gray levels; (picture, residual)"""
    x, y, res = raw_positions(p, w, h, camera)
    with np.errstate(all="ignore"):
        seen = np.clip(np.rint(f(x, y)), 0, 255)
    return np.where(np.isfinite(seen), seen, 0).astype(np.uint8), res


def render_bilinear(p, ideal, w, h, x_offset=0.0, camera=ur.DEFAULT_CAMERA):
    """the raw picture of camera p of the ideal picture `ideal` (an array, sampled bilinearly at (x + x_offset, y), 0 outside)"""
    x, y, _ = raw_positions(p, w, h, camera)
    x = x + x_offset
    H, Wd = ideal.shape
    ok = np.isfinite(x) & np.isfinite(y) & (x >= 0) & (x <= Wd - 1) & (y >= 0) & (y <= H - 1)
    x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    x0, y0 = np.minimum(np.floor(x).astype(np.int64), Wd - 2), np.minimum(np.floor(y).astype(np.int64), H - 2)
    ax, ay = x - x0, y - y0
    g = ideal.astype(np.float64)
    v = (1 - ax) * (1 - ay) * g[y0, x0] + ax * (1 - ay) * g[y0, x0 + 1] + (1 - ax) * ay * g[y0 + 1, x0] + ax * ay * g[y0 + 1, x0 + 1]
    return np.where(ok, np.clip(np.rint(v), 0, 255), 0).astype(np.uint8)


_pair = {}


def textured_raw_pair(seed=31):
    """the raw pictures of the rig looking at sr.texture(640 + 20, 480, seed): the ideal left picture is its columns [0, 640), the ideal right one
    the same shifted by 20 columns.  (raw left, raw right, ideal left, ideal right); made once"""
    if seed not in _pair:
        import stereo_ref as sr
        src = sr.texture(RIG_W + RIG_D, RIG_H, seed)
        p0, p1, _ = rig()
        left = render_bilinear(p0, src, RIG_W, RIG_H, 0.0)
        right = render_bilinear(p1, src, RIG_W, RIG_H, float(RIG_D))
        for a in (left, right):
            a.setflags(write=False)
        _pair[seed] = (left, right, np.ascontiguousarray(src[:, :RIG_W]), np.ascontiguousarray(src[:, RIG_D:RIG_D + RIG_W]))
    return _pair[seed]


def tile_boxes(qx, qy, tw=64, th=32, lds=16384):
    """the source bounding box of every output tile, as k_rect_boxes makes it: [tiles_y, tiles_x, 5] = x0a, y0, pitch, rows, staged"""
    h, w = qx.shape
    ty, tx = (h + th - 1) // th, (w + tw - 1) // tw
    out = np.zeros((ty, tx, 5), np.int64)
    for j in range(ty):
        for i in range(tx):
            a, b = qx[j * th:(j + 1) * th, i * tw:(i + 1) * tw], qy[j * th:(j + 1) * th, i * tw:(i + 1) * tw]
            ok = a != OUTSIDE
            if not ok.any():
                out[j, i] = (0, 0, 16, 0, 0)
                continue
            sx, sy = a[ok].astype(np.int64) >> 5, b[ok].astype(np.int64) >> 5
            bx0, bx1, by0, by1 = sx.min(), sx.max(), sy.min(), sy.max()
            x0, x1 = max(bx0, 0), (bx1 + 1 if bx1 < w - 1 else w - 1)
            y0, y1 = max(by0, 0), (by1 + 1 if by1 < h - 1 else h - 1)
            if not (x0 <= x1 and y0 <= y1):
                out[j, i] = (0, 0, 16, 0, 0)
                continue
            x0a = x0 & ~15
            pitch, rows = (x1 - x0a + 16) & ~15, y1 - y0 + 1
            out[j, i] = (x0a, y0, pitch, rows, int(pitch * rows <= lds))
    return out
