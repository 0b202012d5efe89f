"""Subprocess driver of tests/test_gpu_loop_gba.py: renders the loop scene of tests/loop_driver.py, runs tests/cpp/gba_surface.cpp's gba_run
(loaded with ctypes) and writes its outputs and named blobs to an .npz file.  Usage: gba_driver.py <libgba_surface.so> <out.npz>.
Test infrastructure, never imported by the package."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import loop_driver as ld  # noqa: E402

BLOBS = dict(ba_kf_ids=np.int64, ba_point_ids=np.int64, ba_poses=np.float64, ba_poses_out=np.float64, ba_fixed=np.uint8, ba_points=np.float64,
             ba_points_out=np.float64, ba_edge_pose=np.int32, ba_edge_point=np.int32, ba_obs=np.float64, ba_K4=np.float64, ba_huber=np.float64,
             kf_ids=np.int64, kf_before=np.float64, kf_after=np.float64, pt_ids=np.int64, pt_before=np.float64, pt_after=np.float64,
             fused=np.int64, fused_px=np.float64)


def blob(lib, name, dtype):
    p = ctypes.c_void_p()
    n = lib.gba_blob(name.encode(), ctypes.byref(p))
    return np.zeros(0, dtype) if not p.value else np.frombuffer(ctypes.string_at(p.value, n), dtype).copy()


def run(so, s):
    lib = ctypes.CDLL(so)
    lib.gba_blob.restype = ctypes.c_size_t
    lib.gba_blob.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    c = {k: np.ascontiguousarray(v) for k, v in s.items() if k != "vocab"}
    P = lambda k: c[k].ctypes.data_as(ctypes.c_void_p)
    voc = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    out = np.zeros(48)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.gba_run.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, vp, ctypes.c_size_t, vp]
    rc = lib.gba_run(ld.W, ld.H, P("old_bgr"), P("old_depth"), P("old_T"), len(c["old_bgr"]), P("lead_bgr"), P("lead_depth"), P("lead_T"),
                     P("rev_bgr"), P("rev_depth"), P("rev_T"), len(c["rev_bgr"]), P("drift"), ld.MIN_KF_GAP, ld.CONSISTENCY_TH, voc,
                     len(s["vocab"]), out.ctypes.data_as(vp))
    blobs = {k: blob(lib, k, t) for k, t in BLOBS.items()} if rc == 0 and out[0] else {}
    return rc, out, blobs


if __name__ == "__main__":
    s = ld.scenario()
    rc, out, blobs = run(sys.argv[1], s)
    np.savez(sys.argv[2], rc=rc, out=out, **blobs)
    sys.exit(int(rc))
