"""Subprocess driver of tests/test_gpu_relocalize.py and tools/pnp_bench.py: renders a synth sequence, builds a keyframe map and relocalises
kidnapped frames through ygz::Relocalizer (tests/cpp/reloc_surface.cpp, loaded with ctypes), then writes the outputs to an .npz file.
Usage: reloc_driver.py <libreloc_surface.so> <out.npz>.  Test infrastructure, never imported by the package."""
import ctypes
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

W, H = 640, 480
N_FRAMES, KF_STRIDE = 41, 8
QUERIES = [4, 11, 20, 27, 36]                 # between keyframes of the same trajectory
UNSEEN_SEED = 97                              # a frame rendered from another texture


def scenario():
    from ygz_slam_amd import synth
    import fixtures
    seq = synth.Sequence(N_FRAMES, W, H, seed=11, step=0.02)
    kf_idx = list(range(0, N_FRAMES, KF_STRIDE))
    kf_bgr = np.stack([seq.frame(i) for i in kf_idx])
    kf_depth = np.stack([seq.depth(i).astype(np.float32) for i in kf_idx])
    kf_T = np.stack([seq.poses[i] for i in kf_idx])
    q_bgr = [seq.frame(i) for i in QUERIES]
    nx_bgr = [seq.frame(i + 1) for i in QUERIES]
    other = synth.Sequence(N_FRAMES, W, H, seed=UNSEEN_SEED, step=0.02)
    q_bgr.append(other.frame(4)); nx_bgr.append(other.frame(5))
    gt = np.stack([seq.poses[i] for i in QUERIES] + [other.poses[4]])
    gt_next = np.stack([seq.poses[i + 1] for i in QUERIES] + [other.poses[5]])
    return dict(kf_bgr=kf_bgr, kf_depth=kf_depth, kf_T=kf_T, q_bgr=np.stack(q_bgr), nx_bgr=np.stack(nx_bgr), gt=gt, gt_next=gt_next,
                vocab=fixtures.synthetic_vocabulary())


def run(so, s):
    lib = ctypes.CDLL(so)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    kf_bgr, kf_depth, kf_T = [np.ascontiguousarray(s[k]) for k in ("kf_bgr", "kf_depth", "kf_T")]
    q_bgr, nx_bgr = np.ascontiguousarray(s["q_bgr"]), np.ascontiguousarray(s["nx_bgr"])
    voc = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    out = np.zeros((len(q_bgr), 40))
    lib.reloc_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                              ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    t0 = time.perf_counter()
    rc = lib.reloc_run(W, H, P(kf_bgr), P(kf_depth), P(kf_T), len(kf_bgr), P(q_bgr), len(q_bgr), P(nx_bgr), voc, len(s["vocab"]), P(out))
    wall = time.perf_counter() - t0
    # Vocabulary::score of a vocabulary whose header names another scoring type (L2_NORM = 1): refused, 0
    import struct
    blob = bytearray(s["vocab"]); struct.pack_into("<i", blob, 16, 1)
    w1 = np.array([1, 2], np.uint32); v1 = np.array([0.5, 0.5])
    lib.reloc_score.restype = ctypes.c_double
    b = ctypes.create_string_buffer(bytes(blob), len(blob))
    refused = lib.reloc_score(b, ctypes.c_size_t(len(blob)), P(w1), P(v1), 2, P(w1), P(v1), 2)
    b0 = ctypes.create_string_buffer(s["vocab"], len(s["vocab"]))
    same = lib.reloc_score(b0, ctypes.c_size_t(len(s["vocab"])), P(w1), P(v1), 2, P(w1), P(v1), 2)
    return rc, out, wall, refused, same


if __name__ == "__main__":
    s = scenario()
    rc, out, wall, refused, same = run(sys.argv[1], s)
    np.savez(sys.argv[2], rc=rc, out=out, wall=wall, gt=s["gt"], gt_next=s["gt_next"], refused=refused, same=same)
    sys.exit(int(rc))
