"""k_klt3 keeps a lane's window of the current image between mismatch evaluations while it stays on the same pixels.  The cases of
tests/klt_window_case.py are those on which a stale window, or one mixed up between the three points of a wavefront, would show; their
next_pts, status and err must equal, bit for bit, tests/golden/klt_window_reuse.npz (written by tools/make_klt_window_golden.py with the
build before the window was kept), and the explicit-point cases must agree with the oracle as tests/test_gpu_parity.py asks of LK."""
import numpy as np
import pytest

import klt_window_case as case
from conftest import golden


@pytest.fixture(scope="module")
def tracked(hip_lib):
    return case.track(hip_lib)


@pytest.mark.gpu
def test_kept_window_outputs_bit_identical(tracked):
    out, cells = tracked
    assert case.points_per_pass(cells) < len(case.walk()[0])          # the walk case takes a second pass of the walk over triples
    g = golden("klt_window_reuse")
    assert sorted(out) == sorted(g.files)
    for k in sorted(out):
        ref = g[k]
        assert out[k].dtype == ref.dtype and out[k].shape == ref.shape, k
        assert out[k].tobytes() == ref.tobytes(), "%s: %d of %d bytes differ" % (k, int((out[k].view(np.uint8) != ref.view(np.uint8)).sum()), ref.nbytes)


@pytest.mark.gpu
def test_kept_window_against_oracle(tracked, oracle):
    out, _ = tracked
    imgs, _, _, pts, init = case.small()
    timgs, tpts, tinit = case.tall()
    prm0 = oracle.klt_params()
    prm0.max_level = 0
    runs = [("small_", imgs, pts, init, None), ("level0_", imgs, pts, init, prm0), ("walk_", imgs) + case.walk() + (None,)]
    runs += [("tall%d_" % n, timgs, tpts[:n], tinit[:n], None) for n in (1, 2, 4)]
    for tag, im, p, i, prm in runs:
        oout, ost, _ = oracle.klt_track(im[0], im[1], p, i, prm)
        assert np.array_equal(out[tag + "status"], ost), (tag, np.flatnonzero(out[tag + "status"] != ost))
        m = ost.astype(bool)
        got = out[tag + "pts"]
        # tracks within 1e-5 relative to the track's magnitude, as in test_gpu_parity.py
        assert np.all(np.abs(got[m] - oout[m]).max(1) <= 1e-5 * np.maximum(1.0, np.abs(oout[m]).max(1))), tag
    st = out["small_status"].astype(bool)
    assert not st[7] and st[6] and st[8]             # the textureless point fails between two neighbours that track
    assert np.array_equal(out["small_pts"][3], out["small_pts"][4]) and out["small_err"][3] == out["small_err"][4]      # the identical pair
    st0 = out["level0_status"].astype(bool)
    assert not st0[18] and not st0[21]               # the guesses outside the image, where no coarser level brings them back
