#!/usr/bin/env python3
"""Run ON THE GPU BOX with the build whose outputs are the reference (the commit before k_klt3 kept its window between evaluations):
tracks the cases of tests/klt_window_case.py and writes every output array to the given .npz (tests/golden/klt_window_reuse.npz, read by
tests/test_gpu_klt_window_reuse.py).  Before it tracks anything it confirms on the CPU, with the oracle, that the inputs are worth
tracking: the one-level case has triples in which a point that iterates moves to new pixels while another one stays on its own, and
evaluations at which no point of the triple moves.
The CPU restatement tests/klt_ref.c (order 1) reproduces this output bit for bit without a GPU, the batched_* arrays included: tests/test_klt_ref.py.
usage: tools/make_klt_window_golden.py out.npz"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                 # noqa: E402

import klt_window_case as case     # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402

imgs, _, _, pts, init = case.small()
mixed, moved, kept = case.mixed_evaluations(*case.level0_windows(Oracle(), imgs, pts, init))
print("one-level case, evaluations after the first of a triple: %d mixed, %d on new pixels, %d on kept pixels" % (mixed, moved, kept))
assert mixed >= 3 and moved >= 10 and kept >= 10, (mixed, moved, kept)

from ygz_slam_amd import _lib      # noqa: E402

out, cells = case.track(_lib)
print("cells %d -> %d points per pass" % (cells, case.points_per_pass(cells)))
assert len(pts) <= case.points_per_pass(cells) < len(case.walk()[0]), cells
np.savez_compressed(sys.argv[1], **out)
print({k: (v.shape, int(v.sum()) if v.dtype == np.uint8 else None) for k, v in out.items()})
