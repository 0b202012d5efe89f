"""k_klt3 bit for bit: next_pts, status and err for two of the benchmark's seeded VGA pairs (tests/klt_case.py), once through the batched
path of the step and once from shifted initial guesses, against tests/golden/klt_bitexact.npz (written by tools/make_klt_golden.py with the
build before the evaluation loop was cut down).  Tracks near the convergence tests depend on the last bit of every float sum of the
kernel, so any change of which additions happen, or of their order, shows up here."""
import numpy as np
import pytest

import klt_case
from conftest import golden


@pytest.mark.gpu
def test_klt3_outputs_bit_identical(hip_lib):
    g = golden("klt_bitexact")
    out = klt_case.track(hip_lib)
    assert sorted(out) == sorted(g.files)
    for k in sorted(out):
        ref = g[k]
        assert out[k].dtype == ref.dtype and out[k].shape == ref.shape, k
        assert out[k].tobytes() == ref.tobytes(), "%s: %d of %d values differ" % (k, int((out[k].view(np.uint8) != ref.view(np.uint8)).sum()), ref.size)
