"""The LK tracker on the device against its restatement (tests/klt_ref.c, pinned to the oracle and to both recorded fixtures by
tests/test_klt_ref.py), byte for byte: next_pts, status and err of every case of tests/klt_cases.py through ygz_hip_klt_track, in the order of
the kernel that serves the window (1: k_klt3 for win 21, 2: k_klt<false> otherwise); the exact-sum cases against the oracle itself; the
filtered entry point; the resident batched entry point with non-default parameters; call sequences that exercise the working-image caches
(pad_levels, klt_prep_valid, ygz_ensure_levels); and the refusals.  No comparison carries a tolerance, a mask or a left-out point."""
import numpy as np
import pytest

import klt_cases as kc
import klt_ref

pytestmark = pytest.mark.gpu
I7 = np.array([0, 0, 0, 1.0, 0, 0, 0])


def _ctx(lib, imgs, **kw):
    h, w = imgs[0].shape
    ctx = lib.HipContext(width=w, height=h, levels=3, max_frames=len(imgs), **kw)
    _upload(ctx, imgs)
    return ctx


def _upload(ctx, imgs):
    for s, im in enumerate(imgs):
        ctx.upload_gray(s, im)
    ctx.build_pyramid(0, len(imgs))


def _track(ctx, pts, init, prm):
    return ctx.klt_track(0, 1, pts, init, klt_ref.fill(ctx.klt_params(), **prm))


def _want(pyr, pts, init, prm):
    r = klt_ref.track(pyr[0], pyr[1], pts, init, klt_ref.device_order(prm.get("win", 21)), **prm)
    return r["pts"], r["status"], r["err"]


def _ref(name):
    r = kc.reference(name)
    return r["pts"], r["status"], r["err"]


def _same(got, ref):
    return all(klt_ref.same_bytes(a, b) for a, b in zip(got, ref))


def _check(tag, got, ref, bad):
    if not _same(got, ref):
        bad.append(klt_ref.diff_report(tag, got, ref))


def test_context_refuses_the_shape_below_its_minimum(hip_lib):
    """37 x 29 is below ygz_hip_create's 32 pixels: its cases are held to the oracle on the CPU (tests/test_klt_ref.py), the device runs 37 x 33"""
    assert [p for p in kc.SIZES if not kc.on_device(p)] == ["s37"]
    with pytest.raises(hip_lib.YgzHipError) as e:
        _ctx(hip_lib, kc.pair("s37"))
    assert e.value.code == -1


@pytest.mark.parametrize("pair", sorted(p for p in kc.SIZES if kc.on_device(p)))
def test_every_case_equals_the_restatement(hip_lib, oracle, pair):
    imgs = kc.pair(pair)
    ctx = _ctx(hip_lib, imgs)
    bad = []
    try:
        assert ctx.cells == kc.cells(pair)                     # the count cases are placed around this number
        for name in kc.names(pair):
            _, pts, init, prm = kc.get(name)
            got = _track(ctx, pts, init, prm)
            _check(name, got, _ref(name), bad)
            if kc.is_exact(name):                              # not through the restatement's trees: the oracle itself
                _check(name + " (oracle)", got, oracle.klt_track(imgs[0], imgs[1], pts, init, klt_ref.fill(oracle.klt_params(), **prm)), bad)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def _keep_rule(pts, status, w, h, border):
    """Tracker::TrackKLT's survivor rule on float positions (k_klt_keep)"""
    b, x, y = np.float32(border), pts[:, 0], pts[:, 1]
    return (status != 0) & (x >= b) & (x < np.float32(w - border)) & (y >= b) & (y < np.float32(h - border))


@pytest.mark.parametrize("name", ["filter_w21", "filter_w7"])
def test_filtered_entry_point_on_the_rule_limits(hip_lib, name):
    pr, pts, init, prm = kc.get(name)
    w, h = kc.SIZES[pr]
    ref = _ref(name)
    assert ref[1].all() and klt_ref.same_bytes(ref[0], init)          # max_iter 0: every track ends on its guess, with status 1
    ctx = _ctx(hip_lib, kc.pair(pr))
    bad = []
    try:
        plain = _track(ctx, pts, init, prm)
        _check(name, plain, ref, bad)
        for k, border in enumerate((0, 20)):
            keep = _keep_rule(ref[0], ref[1], w, h, border)
            # the eight guesses placed for this border: on the lower limit (kept), one float below (not), on the upper limit (not), one float below (kept)
            assert keep[8 * k:8 * k + 8].tolist() == [True, False, False, True, True, False, False, True]
            p, st, err, gk, nk = ctx.klt_track_filtered(0, 1, pts, init, border, klt_ref.fill(ctx.klt_params(), **prm))
            _check("%s border %d" % (name, border), (p, st, err), plain, bad)
            assert np.array_equal(gk, keep), (border, np.flatnonzero(gk != keep))
            assert nk == int(keep.sum())
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prm", [dict(win=21, max_level=1, max_iter=5, eps=0.03, min_eig_threshold=1e-3),
                                 dict(win=7, max_level=2, max_iter=10, eps=0.01, min_eig_threshold=0.0)], ids=["win21", "win7"])
def test_resident_batched_tracking_with_non_default_parameters(hip_lib, prm):
    """ygz_hip_track_klt: two pairs (1 <- 0 and 0 <- 1) of detected keypoints; the guess of a track is its reference pixel"""
    imgs = kc.pair("small")
    pyr = kc.pyramids("small")
    ctx = _ctx(hip_lib, imgs)
    bad = []
    try:
        ctx.detect(0, 2)
        cur, ref = [1, 0], [0, 1]
        ctx.track_begin(cur, ref, np.stack([I7, I7]), np.stack([I7, I7]), predict=False)
        ctx.track_klt(klt_ref.fill(ctx.klt_params(), **prm))
        for p in range(2):
            pts = ctx.get_keypoints(ref[p])["px"].astype(np.float32)
            assert len(pts) >= 20
            want = _want((pyr[ref[p]], pyr[cur[p]]), pts, pts, prm)
            _check("pair %d" % p, ctx.track_get_klt(p), want, bad)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def test_call_sequences_in_one_context(hip_lib, oracle):
    """every call of a sequence equals the restatement, whatever the calls before it left in the working-image caches"""
    imgs, pyr = kc.pair("small"), kc.pyramids("small")
    _, pts, init, _ = kc.get("small")
    bad = []

    def play(tag, ctx, seq, pyr=pyr):
        for k, prm in enumerate(seq):
            _check("%s, call %d %r" % (tag, k, prm), _track(ctx, pts, init, prm), _want(pyr, pts, init, prm), bad)

    ctx = _ctx(hip_lib, imgs)
    try:
        play("default / win 7 / default", ctx, [{}, dict(win=7, max_level=1), {}])
    finally:
        ctx.close()
    ctx = _ctx(hip_lib, imgs)
    try:
        play("one level, then more levels than were built", ctx, [dict(max_level=0), dict(win=7, max_level=7), dict(max_level=7), dict(win=3, max_level=7)])
    finally:
        ctx.close()
    ctx = _ctx(hip_lib, imgs)
    try:
        play("before the new frames", ctx, [dict(win=7, max_level=4)])
        new = [imgs[1], np.ascontiguousarray(255 - imgs[0])]              # other pixels in both slots
        _upload(ctx, new)
        new_pyr = (klt_ref.pyramid(oracle, new[0]), klt_ref.pyramid(oracle, new[1]))
        play("after new frames and a rebuilt pyramid", ctx, [dict(max_level=2), dict(win=7, max_level=4), dict(win=15, max_iter=3)], new_pyr)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("prm", [dict(win=7, max_level=4), dict(win=21, max_level=1, max_iter=3), dict(win=20)], ids=["win7", "win21", "win20"])
def test_prepare_then_non_default_track_klt(hip_lib, prm):
    """ygz_hip_track_klt_prepare builds the default tracker's working images; the tracker that follows asks for other levels and windows"""
    imgs, pyr = kc.pair("small"), kc.pyramids("small")
    ctx = _ctx(hip_lib, imgs)
    bad = []
    try:
        ctx.detect(0, 2)
        ctx.track_begin([1], [0], I7[None], I7[None], predict=False)
        ctx.track_klt_prepare()
        ctx.track_klt(klt_ref.fill(ctx.klt_params(), **prm))
        pts = ctx.get_keypoints(0)["px"].astype(np.float32)
        first = _want(pyr, pts, pts, prm)
        _check("prepared, then %r" % prm, ctx.track_get_klt(0), first, bad)
        ctx.track_klt_prepare()                                          # and the default tracker on prepared images after it:
        ctx.track_klt()                                                  # the track set's positions are in / out, it starts from the first result
        _check("prepared, then default", ctx.track_get_klt(0), _want(pyr, pts, first[0], {}), bad)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)


def test_refused_parameters_leave_the_context_usable(hip_lib):
    _, pts, init, _ = kc.get("small")
    ctx = _ctx(hip_lib, kc.pair("small"))
    bad = []
    try:
        _check("before", _track(ctx, pts, init, {}), _ref("small"), bad)
        for prm in (dict(win=2), dict(win=22), dict(max_level=-1), dict(max_level=klt_ref.MAX_LEVELS)):
            with pytest.raises(hip_lib.YgzHipError) as e:
                _track(ctx, pts, init, prm)
            assert e.value.code == -1, prm                               # YGZ_E_INVALID
            _check("after %r" % prm, _track(ctx, pts, init, {}), _ref("small"), bad)
            _check("win 7 after %r" % prm, _track(ctx, pts, init, dict(win=7)), _ref("win7"), bad)
    finally:
        ctx.close()
    assert not bad, "\n".join(bad)
