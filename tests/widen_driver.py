"""Subprocess driver of tests/test_gpu_loop_widen.py: renders the loop scene of tests/loop_driver.py, runs tests/cpp/proj_surface.cpp's
widen_run (loaded with ctypes) and writes its outputs and named blobs to an .npz file.  Usage: widen_driver.py <libproj_surface.so> <out.npz>.
Test infrastructure, never imported by the package."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import loop_driver as ld  # noqa: E402

DTYPES = dict(kp_px=np.float64, kp_level=np.int32, kp_desc=np.uint8, kp_taken=np.uint8, pw=np.float64, pt_desc=np.uint8, pt_dmax=np.float64,
              pt_normal=np.float64, pt_skip=np.uint8, S=np.float64)
PLAIN = dict(K4=np.float64, s3_result=np.int32, sp_result=np.int32, fu_result=np.int32, final=np.int32, cur_px=np.float64, loop_pw=np.float64,
             loop_feature_point=np.int32)


def blob(lib, name, dtype):
    p = ctypes.c_void_p()
    n = lib.widen_blob(name.encode(), ctypes.byref(p))
    return None if not p.value else np.frombuffer(ctypes.string_at(p.value, n), dtype).copy()


def run(so, s):
    lib = ctypes.CDLL(so)
    lib.widen_blob.restype = ctypes.c_size_t
    lib.widen_blob.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
    c = {k: np.ascontiguousarray(v) for k, v in s.items() if k != "vocab"}
    P = lambda k: c[k].ctypes.data_as(ctypes.c_void_p)
    voc = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    out = np.zeros(32)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.widen_run.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, vp, ctypes.c_size_t, vp]
    rc = lib.widen_run(ld.W, ld.H, P("old_bgr"), P("old_depth"), P("old_T"), len(c["old_bgr"]), P("lead_bgr"), P("lead_depth"), P("lead_T"),
                       P("rev_bgr"), P("rev_depth"), P("rev_T"), len(c["rev_bgr"]), P("drift"), ld.MIN_KF_GAP, ld.CONSISTENCY_TH, voc,
                       len(s["vocab"]), out.ctypes.data_as(vp))
    blobs = {}
    if rc == 0 and out[0]:
        for k, t in PLAIN.items():
            blobs[k] = blob(lib, k, t)
        for prefix in ["s3a_", "s3b_", "sp_"] + ["fu%d_" % k for k in range(int(out[16]))]:
            for k, t in DTYPES.items():
                a = blob(lib, prefix + k, t)
                if a is not None:
                    blobs[prefix + k] = a
    return rc, out, blobs


if __name__ == "__main__":
    s = ld.scenario()
    rc, out, blobs = run(sys.argv[1], s)
    # the scene's own constants for the geometric check: the nearest depth any keyframe sees
    zmin = float(min(s["old_depth"][s["old_depth"] > 0].min(), s["rev_depth"][s["rev_depth"] > 0].min()))
    np.savez(sys.argv[2], rc=rc, out=out, rev_T=s["rev_T"], old_T=s["old_T"], drift=s["drift"], zmin=zmin, **blobs)
    sys.exit(int(rc))
