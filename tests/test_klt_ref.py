"""The restatement of the LK tracker (tests/klt_ref.c) is pinned without a tolerance, on the CPU:
  - order 0 (sequential sums) equals the oracle's yo_klt_track on every case of tests/klt_cases.py, byte for byte: the transcription is right;
  - order 1 (k_klt3's lane sums and 21-lane tree) reproduces both recorded fixtures, tests/golden/klt_bitexact.npz and klt_window_reuse.npz,
    byte for byte, from inputs regenerated with the oracle's gray conversion, pyramid and extractor.  That includes klt_window_reuse's three
    batched_* arrays: k_track_load hands the tracker the reference pixel itself as the guess (the predicted pixel goes to the direct projection),
    so no pose enters;
  - on the exact-sum cases every partial sum is an integer below 2^24, and orders 0, 1 / 2 and the oracle agree byte for byte;
  - the cases reach what they are meant to reach (from the restatement's exit taps): every exit at level 0 for both kernel forms, the coarse-level
    exits above level 0, every exit in each position of a win-21 triple beside two points that iterate.
Order 2 (k_klt<false>, ygz_wave_sum_f's association) rests on the reading of the code alone here; tests/test_gpu_klt_ref.py runs it on the device."""
import numpy as np
import pytest

import klt_case
import klt_cases as kc
import klt_ref
import klt_window_case as wc
from conftest import golden


def _triple(r):
    return r["pts"], r["status"], r["err"]


def _assert_same(tag, got, ref):
    assert all(klt_ref.same_bytes(a, b) for a, b in zip(got, ref)), klt_ref.diff_report(tag, got, ref)


@pytest.mark.parametrize("pair", sorted(kc.SIZES))
def test_order0_equals_oracle(oracle, pair):
    imgs = kc.pair(pair)
    assert kc.names(pair)
    for name in kc.names(pair):
        _, pts, init, prm = kc.get(name)
        want = oracle.klt_track(imgs[0], imgs[1], pts, init, klt_ref.fill(oracle.klt_params(), **prm))
        _assert_same(name, _triple(kc.reference(name, 0)), want)


def test_walk_candidates_are_those_of_the_window_case():
    pts, init = kc.walk_candidates()
    assert len(pts) == 100
    keep = np.setdiff1d(np.arange(100), wc.WALK_LEFT_OUT)[:76]
    wp, wi = wc.walk()
    assert klt_ref.same_bytes(pts[keep], wp) and klt_ref.same_bytes(init[keep], wi)


def _check_fixture(g, tag, r):
    for k in ("pts", "status", "err"):
        ref = g[tag + k]
        assert klt_ref.same_bytes(r[k], ref), "%s%s: %d of %d bytes differ" % (tag, k, int((r[k].view(np.uint8) != ref.view(np.uint8)).sum()) if r[k].shape == ref.shape else -1, ref.nbytes)


def test_order1_reproduces_klt_bitexact(oracle):
    """all 12 arrays of klt_bitexact.npz (3,874 tracks), recorded from k_klt3 on the device, from the CPU alone"""
    g = golden("klt_bitexact")
    bgr, _, _ = klt_case.frames()
    gray = [oracle.bgr2gray(b) for b in bgr]
    kps = [oracle.detect(oracle.pyramid(im, klt_case.LEVELS)) for im in gray]
    assert [len(k) for k in kps[:2]] == [996, 941]
    pyr = [klt_ref.pyramid(oracle, im) for im in gray]
    rng = np.random.default_rng(17)
    seen = []
    for p, (c, r) in enumerate(zip(klt_case.CUR, klt_case.REF)):
        pts = np.stack([kps[r]["px"], kps[r]["py"]], 1).astype(np.float32)
        _check_fixture(g, "batched_%d_" % p, klt_ref.track(pyr[r], pyr[c], pts, pts, 1))
        seen += ["batched_%d_" % p]
    for p, (c, r) in enumerate(zip(klt_case.CUR, klt_case.REF)):
        pts = np.stack([kps[r]["px"], kps[r]["py"]], 1).astype(np.float32)
        init = pts + rng.uniform(-2.0, 2.0, pts.shape).astype(np.float32)
        _check_fixture(g, "shifted_%d_" % p, klt_ref.track(pyr[r], pyr[c], pts, init, 1))
        seen += ["shifted_%d_" % p]
    assert sorted(g.files) == sorted(t + k for t in seen for k in ("pts", "status", "err"))


def test_order1_reproduces_klt_window_reuse(oracle):
    """all 21 arrays of klt_window_reuse.npz, the batched_* ones included (their guesses are the detected reference pixels themselves)"""
    g = golden("klt_window_reuse")
    seen = []
    for tag, name in [("small_", "small"), ("level0_", "level0_w21"), ("walk_", "walk"), ("tall1_", "tall1"), ("tall2_", "tall2"), ("tall4_", "tall4")]:
        _check_fixture(g, tag, kc.reference(name))
        seen.append(tag)
    assert np.flatnonzero(g["small_status"] == 0).size + np.flatnonzero(g["level0_status"] == 0).size + np.flatnonzero(g["walk_status"] == 0).size == 22
    imgs = kc.pair("small")
    kp = oracle.detect(oracle.pyramid(imgs[0], 3))
    pts = np.stack([kp["px"], kp["py"]], 1).astype(np.float32)
    assert len(pts) == len(g["batched_status"])
    pl, nl = kc.pyramids("small")
    _check_fixture(g, "batched_", klt_ref.track(pl, nl, pts, pts, 1))         # pair (cur 1, ref 0): reference frame 0, searched frame 1
    seen.append("batched_")
    assert sorted(g.files) == sorted(t + k for t in seen for k in ("pts", "status", "err"))


@pytest.mark.parametrize("name", [n for n in kc.names() if kc.is_exact(n)])
def test_exact_sum_cases_agree_in_every_order(oracle, name):
    pr, pts, init, prm = kc.get(name)
    imgs = kc.pair(pr)
    dev = kc.reference(name)
    seq = kc.reference(name, 0)
    for r in (dev, seq):
        assert r["max_sum"].max() < 2.0 ** 24, r["max_sum"].max()
    assert (dev["iters"].sum(1) >= 2).sum() >= len(pts) // 2                 # the sums are not trivially zero: most points iterate
    assert dev["status"].any()
    want = oracle.klt_track(imgs[0], imgs[1], pts, init, klt_ref.fill(oracle.klt_params(), **prm))
    _assert_same(name + " (sequential)", _triple(seq), want)
    _assert_same(name + " (device order)", _triple(dev), want)
    for k in ("exit", "iters", "min_eig"):
        assert klt_ref.same_bytes(dev[k], seq[k]), k


# ---- what the cases reach, from the restatement alone --------------------------------------------------------------------------------------
def _exit_sets(names):
    lvl0, coarse = set(), set()
    for n in names:
        r = kc.reference(n)
        lvl0 |= set(int(c) for c in r["exit"][:, 0])
        coarse |= set(int(c) for c in r["exit"][:, 1:].ravel())
        # a guess window that leaves the image WHILE iterating: after at least one evaluation
        if ((r["exit"][:, 0] == klt_ref.GUESS_OUT) & (r["iters"][:, 0] >= 1)).any():
            lvl0.add("left at j >= 1")
        if ((r["exit"][:, 1:] == klt_ref.GUESS_OUT) & (r["iters"][:, 1:] >= 1)).any():
            coarse.add("left at j >= 1")
    return lvl0, coarse


@pytest.mark.parametrize("win", kc.KERNEL_WINS)
def test_cases_reach_every_exit_per_kernel_form(win):
    lvl0, coarse = _exit_sets([n for n in kc.names() if kc.get(n)[3].get("win", 21) == win])
    assert set(klt_ref.EXITS) | {"left at j >= 1"} <= lvl0, [klt_ref.EXIT_NAMES[c] for c in klt_ref.EXITS if c not in lvl0]
    assert set(klt_ref.COARSE_EXITS) | {"left at j >= 1"} <= coarse, [klt_ref.EXIT_NAMES[c] for c in klt_ref.COARSE_EXITS if c not in coarse]


@pytest.mark.parametrize("win", kc.KERNEL_WINS)
def test_exit_points_reach_their_exit(win):
    r = kc.reference("exits_w%d" % win)
    for k, c in enumerate(klt_ref.EXITS):
        assert r["exit"][k, 0] == c, (klt_ref.EXIT_NAMES[c], klt_ref.EXIT_NAMES[r["exit"][k, 0]])
    k = klt_ref.EXITS.index(klt_ref.GUESS_OUT)
    assert r["iters"][k, 0] >= 1
    assert kc.reference("err_out_w15")["exit"][:3, 0].tolist() == [klt_ref.ERR_OUT] * 3


def test_triples_hold_every_exit_in_every_position():
    r = kc.reference("triple")
    ex, it = r["exit"][:, 0], r["iters"][:, 0]
    assert len(ex) == 63
    seen = set()
    for t in range(0, 63, 3):
        c, k = klt_ref.EXITS[t // 9], (t // 3) % 3
        assert ex[t + k] == c, (klt_ref.EXIT_NAMES[c], k, klt_ref.EXIT_NAMES[ex[t + k]])
        for o in range(3):
            if o != k:                                                      # the neighbours iterate normally
                assert ex[t + o] in (klt_ref.CONVERGED, klt_ref.OSCILLATION) and it[t + o] >= 3 and r["status"][t + o] == 1
        seen.add((c, k))
    assert len(seen) == 21


def test_border_cases_sit_on_the_limits():
    for win in kc.KERNEL_WINS:
        ref_kept = [klt_ref.REF_OUT != c for c in kc.reference("border_l0_w%d" % win)["exit"][:, 0]]
        assert ref_kept == [True, False, True, False, True, False, True, False, True], (win, ref_kept)
        r = kc.reference("guess_border_w%d" % win)
        out0 = [(c == klt_ref.GUESS_OUT and j == 0) for c, j in zip(r["exit"][:, 0], r["iters"][:, 0])]
        assert out0 == [False, True, False, True, False, True, False, True, False], (win, out0)
        assert (r["iters"][0::2, 0] >= 1).all()                            # on the limit itself the window is evaluated


def test_mineig_threshold_on_the_value_and_one_float_above():
    for win in kc.KERNEL_WINS:
        at, above = kc.reference("mineig_at_w%d" % win), kc.reference("mineig_above_w%d" % win)
        thr = np.float32(kc.get("mineig_at_w%d" % win)[3]["min_eig_threshold"])
        assert at["min_eig"][1, 0] == thr and at["exit"][1, 0] != klt_ref.EIG_FAIL and at["status"][1] == 1
        assert above["min_eig"][1, 0] == thr and above["exit"][1, 0] == klt_ref.EIG_FAIL and above["status"][1] == 0
        assert np.float32(kc.get("mineig_above_w%d" % win)[3]["min_eig_threshold"]) == np.nextafter(thr, np.float32(np.inf))


def test_checkerboard_is_flattened_by_pyr_down():
    pl, _ = kc.pyramids("checker")
    assert np.all(pl[1] == 128) and len(np.unique(pl[0])) > 50
    for win in kc.KERNEL_WINS:
        r = kc.reference("checker_w%d" % win)
        assert r["levels"] == 2
        assert (r["exit"][:, 1] == klt_ref.EIG_FAIL).all()                  # the coarse level is skipped
        assert r["status"][0] == 1 and r["exit"][0, 0] in (klt_ref.CONVERGED, klt_ref.OSCILLATION, klt_ref.MAX_ITER)     # level 0 tracks


def test_parameter_cases_take_their_clamps():
    for win in kc.KERNEL_WINS:
        t = "_w%d" % win
        assert _triple(kc.reference("iter-1" + t))[0].tobytes() == _triple(kc.reference("iter0" + t))[0].tobytes()
        assert kc.reference("iter0" + t)["iters"].max() == 0
        assert kc.reference("iter101" + t)["iters"].max() <= 100
        _assert_same("max_iter 101 is 100", _triple(kc.reference("iter101" + t)), _triple(kc.reference("iter100" + t)))
        _assert_same("eps -1 is 0", _triple(kc.reference("eps0" + t)), _triple(kc.reference("eps1" + t)))
        _assert_same("eps 11 is 10", _triple(kc.reference("eps5" + t)), _triple(kc.reference("eps4" + t)))
        assert not kc.reference("thr2" + t)["status"].any()                 # above every patch's eigenvalue
        assert kc.reference("noflow" + t)["status"].sum() >= 15             # the far guesses were ignored
        assert [kc.reference("level%d%s" % (m, t))["levels"] for m in (0, 1, 2, 4, 7)] == ([1, 2, 3, 3, 3] if win == 21 else [1, 2, 3, 5, 5])
    assert kc.reference("win3_level7")["levels"] == 6 and kc.reference("tall_level7_w7")["levels"] == 6
    assert kc.reference("shape_s37_w21")["levels"] == 1 and kc.reference("shape_s37x33_w21")["levels"] == 1 and kc.reference("shape_tall_w21")["levels"] == 5
