"""Subprocess driver of tests/test_gpu_loop_correct.py: renders the loop scene of tests/loop_driver.py, runs tests/cpp/correct_surface.cpp's
correct_run (loaded with ctypes) and writes its outputs and named blobs to an .npz file.  Usage: correct_driver.py <libcorrect_surface.so>
<out.npz>.  Test infrastructure, never imported by the package."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import loop_driver as ld  # noqa: E402

BLOBS = dict(K4=np.float64, S_cw=np.float64, kf_ids=np.int32, pt_kf=np.int32, pt_px=np.float64, poses_before=np.float64, poses_after=np.float64,
             pt_before=np.float64, pt_after=np.float64, left_out=np.int32, g_ids=np.int32, g_S=np.float64, g_S_out=np.float64, g_fixed=np.uint8,
             g_edges=np.int32, g_M=np.float64)


def blob(lib, name, dtype):
    p = ctypes.c_void_p()
    n = lib.correct_blob(name.encode(), ctypes.byref(p))
    return np.zeros(0, dtype) if not p.value else np.frombuffer(ctypes.string_at(p.value, n), dtype).copy()


def run(so, s):
    lib = ctypes.CDLL(so)
    lib.correct_blob.restype = ctypes.c_size_t
    lib.correct_blob.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    c = {k: np.ascontiguousarray(v) for k, v in s.items() if k != "vocab"}
    P = lambda k: c[k].ctypes.data_as(ctypes.c_void_p)
    voc = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    out = np.zeros(32)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.correct_run.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, vp, ctypes.c_size_t, vp]
    rc = lib.correct_run(ld.W, ld.H, P("old_bgr"), P("old_depth"), P("old_T"), len(c["old_bgr"]), P("lead_bgr"), P("lead_depth"), P("lead_T"),
                         P("rev_bgr"), P("rev_depth"), P("rev_T"), len(c["rev_bgr"]), P("drift"), ld.MIN_KF_GAP, ld.CONSISTENCY_TH, voc,
                         len(s["vocab"]), out.ctypes.data_as(vp))
    blobs = {k: blob(lib, k, t) for k, t in BLOBS.items()} if rc == 0 and out[0] else {}
    return rc, out, blobs


if __name__ == "__main__":
    s = ld.scenario()
    rc, out, blobs = run(sys.argv[1], s)
    np.savez(sys.argv[2], rc=rc, out=out, rev_T=s["rev_T"], old_T=s["old_T"], lead_T=s["lead_T"], drift=s["drift"], **blobs)
    sys.exit(int(rc))
