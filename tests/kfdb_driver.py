"""Subprocess driver of tests/test_gpu_kfdb_surface.py: the scenes of tests/loop_driver.py and tests/reloc_driver.py, each run through
tests/cpp/kfdb_surface.cpp (loaded with ctypes) three times -- without a ygz::KeyFrameDatabase, with one that holds every keyframe and with
one that holds every second keyframe -- and the outputs written to an .npz file.  Usage: kfdb_driver.py <libkfdb_surface.so> <out.npz>.
Test infrastructure, never imported by the package."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import loop_driver
import reloc_driver

MODES = (0, 1, 2)                             # no database, every keyframe, every second keyframe


def run_loop(lib, s, mode):
    c = {k: np.ascontiguousarray(v) for k, v in s.items() if k != "vocab"}
    P = lambda k: c[k].ctypes.data_as(ctypes.c_void_p)
    voc = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    n_rev, n_oth = len(c["rev_bgr"]), len(c["oth_bgr"])
    out, checks = np.zeros((n_rev + n_oth, 256)), np.zeros(16)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.kfdb_loop_run.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp, ctypes.c_size_t, ci, vp, vp]
    rc = lib.kfdb_loop_run(loop_driver.W, loop_driver.H, P("old_bgr"), P("old_depth"), P("old_T"), len(c["old_bgr"]), P("lead_bgr"),
                           P("lead_depth"), P("lead_T"), P("rev_bgr"), P("rev_depth"), P("rev_T"), n_rev, P("drift"), P("oth_bgr"),
                           P("oth_depth"), P("oth_T"), n_oth, loop_driver.MIN_KF_GAP, loop_driver.CONSISTENCY_TH, voc, len(s["vocab"]), mode,
                           out.ctypes.data_as(vp), checks.ctypes.data_as(vp))
    return rc, out, checks


def run_reloc(lib, s, mode):
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    kf_bgr, kf_depth, kf_T, q_bgr = [np.ascontiguousarray(s[k]) for k in ("kf_bgr", "kf_depth", "kf_T", "q_bgr")]
    voc = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    out = np.zeros((len(q_bgr), 40))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.kfdb_reloc_run.argtypes = [ci, ci, vp, vp, vp, ci, vp, ci, vp, ctypes.c_size_t, ci, vp]
    rc = lib.kfdb_reloc_run(reloc_driver.W, reloc_driver.H, P(kf_bgr), P(kf_depth), P(kf_T), len(kf_bgr), P(q_bgr), len(q_bgr), voc,
                            len(s["vocab"]), mode, P(out))
    return rc, out


if __name__ == "__main__":
    lib = ctypes.CDLL(sys.argv[1])
    res, rc = {}, 0
    s = loop_driver.scenario()
    for m in MODES:
        r, out, checks = run_loop(lib, s, m)
        rc = rc or r
        res["loop%d" % m] = out
        if m == 1:
            res["checks"] = checks
    s = reloc_driver.scenario()
    for m in MODES:
        r, out = run_reloc(lib, s, m)
        rc = rc or r
        res["reloc%d" % m] = out
    np.savez(sys.argv[2], rc=rc, n_rev=len(loop_driver.REVISIT), **res)
    sys.exit(int(rc))
