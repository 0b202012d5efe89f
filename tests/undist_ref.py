"""ctypes loader of tests/undist_ref.c, the restatement of the undistortion stage (ygz_slam_amd/csrc/undistort.hip) that
tests/test_undist_ref.py holds to a numpy witness and tests/test_gpu_undistort.py holds the map and the image of the device against.  Test
infrastructure: compiled with gcc into a temporary directory the first time it is used, never imported by the package.  Also the cameras and
pictures both tests share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

OUTSIDE = -2 ** 31
# the context's default camera (ygz_hip_default_params: config/default.yaml) as the floats it stores, converted to double
DEFAULT_CAMERA = tuple(float(np.float32(v)) for v in (520.9, 521.0, 325.1, 249.7))
TUM_FR1 = dict(k1=0.2624, k2=-0.9531, p1=-0.0054, p2=0.0026, k3=1.1633)          # the TUM RGB-D fr1 calibration


class Params(ctypes.Structure):
    """ur_params = ygz_undistort_params"""
    _fields_ = [("k1", ctypes.c_double), ("k2", ctypes.c_double), ("p1", ctypes.c_double), ("p2", ctypes.c_double), ("k3", ctypes.c_double),
                ("fx", ctypes.c_double), ("fy", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("border_value", ctypes.c_int)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="undist_ref_")
        so = os.path.join(d, "libundist_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "undist_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        dbl = ctypes.c_double
        _lib.ur_map.argtypes = [ctypes.c_int, ctypes.c_int, dbl, dbl, dbl, dbl, ctypes.POINTER(Params), ctypes.POINTER(ctypes.c_int32),
                                ctypes.POINTER(ctypes.c_int32)]
        _lib.ur_map_real.argtypes = [ctypes.c_int, ctypes.c_int, dbl, dbl, dbl, dbl, ctypes.POINTER(Params), ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
        _lib.ur_remap.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                                  ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)]
        _lib.ur_distort_point.argtypes = [ctypes.POINTER(Params), dbl, dbl, ctypes.POINTER(dbl), ctypes.POINTER(dbl)]
        for f in (_lib.ur_map, _lib.ur_map_real, _lib.ur_remap, _lib.ur_distort_point):
            f.restype = None
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(camera=DEFAULT_CAMERA, border_value=0, **coeff):
    """zero coefficients, the source camera = `camera` (fx, fy, cx, cy) unless fx .. cy are given"""
    v = dict(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, fx=camera[0], fy=camera[1], cx=camera[2], cy=camera[3])
    v.update(coeff)
    return Params(*[float(v[k]) for k in ("k1", "k2", "p1", "p2", "k3", "fx", "fy", "cx", "cy")], int(border_value))


def fields(p):
    return {n: getattr(p, n) for n, _ in Params._fields_}


def build_map(w, h, p, camera=DEFAULT_CAMERA):
    """ur_map: (qx, qy) [h, w] int32 for the output camera `camera`"""
    qx, qy = np.empty((h, w), np.int32), np.empty((h, w), np.int32)
    lib().ur_map(w, h, *[float(c) for c in camera], ctypes.byref(p), _p(qx, ctypes.c_int32), _p(qy, ctypes.c_int32))
    return qx, qy


def map_real(w, h, p, camera=DEFAULT_CAMERA):
    mx, my = np.empty((h, w), np.float64), np.empty((h, w), np.float64)
    lib().ur_map_real(w, h, *[float(c) for c in camera], ctypes.byref(p), _p(mx, ctypes.c_double), _p(my, ctypes.c_double))
    return mx, my


def remap(src, qx, qy, border_value=0):
    """ur_remap: src [h, w] gray or [h, w, 3] BGR"""
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape[:2]
    ch = 1 if src.ndim == 2 else 3
    assert qx.shape == qy.shape == (h, w) and (src.ndim == 2 or src.shape[2] == 3)
    out = np.empty((h, w), np.uint8)
    lib().ur_remap(w, h, _p(src, ctypes.c_uint8), ch, _p(np.ascontiguousarray(qx), ctypes.c_int32), _p(np.ascontiguousarray(qy), ctypes.c_int32),
                   int(border_value), _p(out, ctypes.c_uint8))
    return out


def undistort(src, p, camera=DEFAULT_CAMERA):
    h, w = src.shape[:2]
    qx, qy = build_map(w, h, p, camera)
    return remap(src, qx, qy, p.border_value)


def distort_point(p, x, y):
    xd, yd = ctypes.c_double(0), ctypes.c_double(0)
    lib().ur_distort_point(ctypes.byref(p), float(x), float(y), ctypes.byref(xd), ctypes.byref(yd))
    return xd.value, yd.value


def picture(w, h, seed, channels=1):
    """a seeded picture with structure at every scale: smooth waves plus noise, so that a wrong tap or weight changes the result"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    shape = (h, w) if channels == 1 else (h, w, 3)
    base = 127.5 + 80.0 * np.sin(x / 7.0 + seed) * np.cos(y / 5.0)
    img = (base if channels == 1 else base[:, :, None]) + rng.integers(-40, 41, shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def gray_of(bgr):
    b, g, r = [bgr[..., k].astype(np.int64) for k in range(3)]
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)
