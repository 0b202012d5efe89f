#!/usr/bin/env python3
"""Run ON THE GPU BOX with the build whose outputs are the reference: tracks tests/klt_case.py's two seeded VGA pairs with the batched
LK path (k_klt3) and writes every output array to the given .npz (tests/golden/klt_bitexact.npz, read by tests/test_gpu_klt_bitexact.py).
The CPU restatement tests/klt_ref.c (order 1) reproduces this output bit for bit without a GPU: tests/test_klt_ref.py.
usage: tools/make_klt_golden.py out.npz"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np                 # noqa: E402

import klt_case                    # noqa: E402
from ygz_slam_amd import _lib      # noqa: E402

out = klt_case.track(_lib)
np.savez_compressed(sys.argv[1], **out)
print({k: (v.shape, int(v.sum()) if v.dtype == np.uint8 else None) for k, v in out.items()})
