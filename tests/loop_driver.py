"""Subprocess driver of tests/test_gpu_loop_closing.py and tools/sim3_bench.py: renders synth sequences, builds an old keyframe map and a
revisit run in a drifted world, hands each revisit keyframe to ygz::LoopClosing (tests/cpp/loop_surface.cpp, loaded with ctypes), then a
run of another texture, and writes the outputs to an .npz file.  Usage: loop_driver.py <libloop_surface.so> <out.npz>.  Test
infrastructure, never imported by the package."""
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

W, H = 640, 480
SEED, OTHER_SEED = 11, 97
OLD = list(range(0, 40, 4))                   # the old run: keyframe ids 0 .. 9
REVISIT = [2, 6, 10, 14, 18, 22]              # the revisit run after its lead keyframe (id 10): ids 11 .. 16
OTHER = [0, 4, 8, 12, 16]                     # another texture: ids 17 .. 21
MIN_KF_GAP, CONSISTENCY_TH = 10, 3            # the defaults
# the drift D of the revisit run's world: s_d = 1.2, about 4 degrees, about 10 cm
DRIFT_AXIS, DRIFT_DEG, DRIFT_T, DRIFT_S = np.array([0.3, -0.8, 0.5]), 4.0, np.array([0.06, -0.05, 0.06]), 1.2


def drift():
    a = DRIFT_AXIS / np.linalg.norm(DRIFT_AXIS)
    h = np.deg2rad(DRIFT_DEG) / 2
    return np.concatenate([a * np.sin(h), [np.cos(h)], DRIFT_T, [DRIFT_S]])


def scenario():
    from ygz_slam_amd import synth
    import fixtures
    n = max(OLD + REVISIT) + 1
    seq = synth.Sequence(n, W, H, seed=SEED, step=0.02)
    oth = synth.Sequence(max(OTHER) + 2, W, H, seed=OTHER_SEED, step=0.02)
    stack = lambda s, idx, f: np.stack([f(s, i) for i in idx])
    bgr, dep = (lambda s, i: s.frame(i)), (lambda s, i: s.depth(i).astype(np.float32))
    return dict(old_bgr=stack(seq, OLD, bgr), old_depth=stack(seq, OLD, dep), old_T=seq.poses[OLD],
                lead_bgr=oth.frame(max(OTHER) + 1), lead_depth=oth.depth(max(OTHER) + 1).astype(np.float32), lead_T=oth.poses[max(OTHER) + 1],
                rev_bgr=stack(seq, REVISIT, bgr), rev_depth=stack(seq, REVISIT, dep), rev_T=seq.poses[REVISIT],
                oth_bgr=stack(oth, OTHER, bgr), oth_depth=stack(oth, OTHER, dep), oth_T=oth.poses[OTHER],
                drift=drift(), vocab=fixtures.synthetic_vocabulary())


def run(so, s):
    lib = ctypes.CDLL(so)
    c = {k: np.ascontiguousarray(v) for k, v in s.items() if k != "vocab"}
    P = lambda k: c[k].ctypes.data_as(ctypes.c_void_p)
    voc = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    n_rev, n_oth = len(c["rev_bgr"]), len(c["oth_bgr"])
    out = np.zeros((n_rev + n_oth, 40))
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.loop_run.argtypes = [ci, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp, ctypes.c_size_t, vp]
    t0 = time.perf_counter()
    rc = lib.loop_run(W, H, P("old_bgr"), P("old_depth"), P("old_T"), len(c["old_bgr"]), P("lead_bgr"), P("lead_depth"), P("lead_T"),
                      P("rev_bgr"), P("rev_depth"), P("rev_T"), n_rev, P("drift"), P("oth_bgr"), P("oth_depth"), P("oth_T"), n_oth, MIN_KF_GAP,
                      CONSISTENCY_TH, voc, len(s["vocab"]), out.ctypes.data_as(vp))
    wall = time.perf_counter() - t0
    return rc, out, wall


if __name__ == "__main__":
    s = scenario()
    rc, out, wall = run(sys.argv[1], s)
    np.savez(sys.argv[2], rc=rc, out=out, wall=wall, old_T=s["old_T"], rev_T=s["rev_T"], drift=s["drift"], n_rev=len(REVISIT))
    sys.exit(int(rc))
