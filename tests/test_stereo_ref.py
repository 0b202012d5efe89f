"""The restatement of the stereo stage (tests/stereo_ref.c, the yardstick the device is held to bit for bit in tests/test_gpu_stereo.py) against a
numpy witness of the same spec written another way, on the scenes of tests/stereo_ref.py; the bounds that follow from the spec (delta in
(-1/2, 1/2], a twin found within half a level pixel of the pictures' shift); and the conditions the scenes are built to meet: every status code
occurs, the interior of the three-level shift scene is all OK, the noise scene splits into MEDIAN and OK, the offset twins give EDGE and k = -4,
the mirror picture takes the 0.01 branch.  No device."""
import numpy as np
import pytest

import stereo_ref as sr

SCENES = ["a", "b", "c", "d", "e"]
VARIANTS = {"default": {}, "window": dict(min_disparity=7.5, max_disparity=27.0, th_dist=50, baseline=0.537)}


@pytest.fixture(scope="module")
def results(oracle):
    out = {}
    for name in SCENES:
        s = sr.scene(oracle, name)
        out[name] = (s, sr.match(s.left, s.right, s.kl, s.kr, sr.params()))
    return out


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("name", SCENES)
def test_restatement_equals_the_witness(oracle, results, name, variant):
    s = results[name][0]
    p = sr.params(**VARIANTS[variant])
    r = results[name][1] if variant == "default" else sr.match(s.left, s.right, s.kl, s.kr, p)
    w = sr.witness(s.left, s.right, s.kl, s.kr, p)
    assert sorted(r) == sorted(w)
    for key in r:
        assert r[key].dtype == w[key].dtype and np.array_equal(r[key], w[key]), key
    assert r["counts"].sum() == len(s.kl["level"]) and np.array_equal(r["counts"], np.bincount(r["status"], minlength=sr.N_STATUS))


def test_empty_lists(oracle, results):
    s = results["a"][0]
    none = sr.head(s.kr, 0)
    r = sr.match(s.left, s.right, s.kl, none, sr.params())
    assert (r["status"] == sr.NO_CANDIDATE).all() and (r["n_cand"] == 0).all() and (r["best_idx"] == -1).all() and (r["sads"] == -1).all()
    assert (r["depth"] == -1.0).all() and (r["u_right"] == -1.0).all() and (r["right_idx"] == -1).all() and (r["sad"] == -1).all()
    r = sr.match(s.left, s.right, sr.head(s.kl, 0), s.kr, sr.params())
    assert len(r["status"]) == 0 and not r["counts"].any()


@pytest.mark.parametrize("name", SCENES)
def test_output_conventions_and_derived_bounds(results, name):
    s, r = results[name]
    st = r["status"]
    ok, med = st == sr.OK, st == sr.MEDIAN
    assert ((r["right_idx"] >= 0) == (ok | med)).all() and ((r["sad"] >= 0) == (ok | med)).all()
    assert ((r["u_right"] != -1.0) == ok).all() and ((r["depth"] > 0) == ok).all() and (r["depth"][~ok] == -1.0).all()
    reached = np.isin(st, (sr.OK, sr.MEDIAN, sr.EDGE, sr.DISPARITY))
    assert ((r["sads"] >= 0).all(axis=1) == reached).all() and ((r["sads"] == -1).all(axis=1) == ~reached).all()
    assert (r["sads"] <= 121 * 510).all()
    # delta in (-1/2, 1/2]: d1 > d2 <= d3 at the first minimum
    fitted = np.isin(st, (sr.OK, sr.MEDIAN, sr.DISPARITY))
    assert (r["delta"][fitted] > -0.5).all() and (r["delta"][fitted] <= 0.5).all() and (r["delta"][~fitted] == 0).all()
    # an OK keypoint matched to its twin lies within half a pixel of its level of the pictures' shift (the twins of scene e are displaced on purpose)
    if name != "e":
        twin = ok & (r["right_idx"] == s.twin)
        err = np.abs(s.kl["px"][twin, 0] - r["u_right"][twin] - s.shift)
        assert (err <= 0.5 * np.exp2(s.kl["level"][twin])).all()
        print("scene %s: %d OK at their twin, largest error %.3f level pixels" % (name, twin.sum(), (err / np.exp2(s.kl["level"][twin])).max() if twin.any() else 0))
    # depth = bf / disparity, the disparity 0.01 where that branch was taken
    disp = s.kl["px"][ok, 0] - r["u_right"][ok]
    disp[r["u_right"][ok] == s.kl["px"][ok, 0] - 0.01] = 0.01
    assert np.array_equal(r["depth"][ok], sr.DEFAULT_FX * 0.1 / disp)


def test_every_status_occurs(results):
    seen = np.zeros(sr.N_STATUS, np.int64)
    for name in SCENES:
        seen += results[name][1]["counts"]
    assert (seen > 0).all(), seen


def test_shift_scene_interior_is_all_ok(results):
    s, r = results["a"]
    px, lv = s.kl["px"], s.kl["level"]
    m = 16.0 * np.exp2(lv)
    h, w = s.left[0].shape
    inner = (px[:, 0] - s.shift >= m) & (px[:, 0] < w - m) & (px[:, 1] >= m) & (px[:, 1] < h - m)
    assert inner.sum() > 200 and (r["status"][inner] == sr.OK).all() and (r["right_idx"][inner] == s.twin[inner]).all()
    assert (inner & (lv == 2)).sum() >= 30 and set(lv[inner]) == {0, 1, 2}


def test_noise_scene_splits(results):
    c = results["b"][1]["counts"]
    assert c[sr.MEDIAN] >= 50 and c[sr.OK] >= 50


def test_identical_pictures_give_disparity(results):
    s, r = results["c"]
    assert r["counts"][sr.DISPARITY] >= 20
    d = r["status"] == sr.DISPARITY
    assert (r["delta"][d] > 0).all() and (r["k"][d] == 0).all()                 # the column right of the keypoint: a negative disparity
    z = (r["status"] == sr.OK)
    assert (r["delta"][z] <= 0).all()


def test_mirror_picture_takes_the_small_disparity_branch(results):
    s, r = results["d"]
    c = 16
    assert r["status"][c] == sr.OK and r["k"][c] == 0 and r["delta"][c] == 0.0 and r["sads"][c][4] == r["sads"][c][6]
    assert r["u_right"][c] == 16.0 - 0.01 and r["depth"][c] == sr.DEFAULT_FX * 0.1 / 0.01
    st = r["status"]
    assert (st[:10] == sr.BORDER).all() and (st[24:] == sr.BORDER).all() and (st[10:24] != sr.BORDER).all()      # sr in [10, 23] is the only legal strip


def test_offset_twins(results):
    s, r = results["e"]
    have = np.nonzero(s.twin >= 0)[0]
    assert np.array_equal(r["best_idx"][have], s.twin[have]) and (r["best_dist"][have] == 0).all()          # never the repeated copy at the end
    assert (s.twin[have] < 8).sum() == 8
    reached = have[r["status"][have] != sr.BORDER]
    even, odd = reached[reached % 2 == 0], reached[reached % 2 == 1]
    assert len(even) > 100 and (r["status"][even] == sr.EDGE).all() and (r["k"][even] == -sr.L).all()
    assert len(odd) > 100 and (r["status"][odd] == sr.OK).all() and (r["k"][odd] == -4).all() and (r["sad"][odd] == 0).all()


@pytest.mark.parametrize("status, sad", [
    ([], []),                                                                  # m = 0, n = 0
    ([sr.BORDER, sr.EDGE], [-1, -1]),                                          # m = 0
    ([sr.OK], [700]),                                                          # m = 1
    ([sr.OK, sr.OK], [100, 211]),                                              # m = 2: med = the larger
    ([sr.OK, sr.OK], [211, 100]),
    ([sr.OK, sr.BORDER, sr.OK, sr.OK], [10, -1, 21, 22]),                      # odd m: med 21
    ([sr.OK, sr.OK, sr.OK, sr.OK], [10, 21, 22, 5]),                           # even m: med = element 2 of (5, 10, 21, 22)
    ([sr.OK, sr.OK, sr.OK, sr.OK, sr.OK], [100, 100, 100, 210, 211]),          # 10 * 210 = 21 * 100 stays
    ([sr.OK] * 6, [55] * 6),                                                   # all equal
    ([sr.OK, sr.OK, sr.OK, sr.DISPARITY], [0, 0, 1, -1]),                      # med = 0: zero stays, the rest goes
    ([sr.OK] * 4, [0, 0, 0, 0]),                                               # a perfect pair keeps every match
    ([sr.OK] * 3, [61710, 0, 61710]),                                          # the largest sum there is
])
def test_median_rule(status, sad):
    got, counts = sr.median_rule(status, sad)
    want, wcounts = sr.witness_median(status, sad)
    assert np.array_equal(got, want) and np.array_equal(counts, wcounts)
    st, sd = np.array(status, np.int64), np.array(sad, np.int64)
    ok = st == sr.OK
    if ok.any():
        med = sorted(sd[ok])[int(ok.sum()) // 2]
        assert np.array_equal(got == sr.MEDIAN, ok & (10 * sd > 21 * med))
    else:
        assert np.array_equal(got, st)


def test_median_rule_examples():
    assert list(sr.median_rule([0, 0], [100, 211])[0]) == [0, 0]
    assert list(sr.median_rule([0, 0, 0, 0, 0], [100, 100, 100, 210, 211])[0]) == [0, 0, 0, 0, 6]
    assert list(sr.median_rule([0, 0, 0, 5], [0, 0, 1, -1])[0]) == [0, 0, 6, 5]
    assert list(sr.median_rule([0, 0, 0, 0], [10, 21, 22, 5])[0]) == [0, 0, 0, 0]           # med 21
    assert list(sr.median_rule([0, 0, 0, 0], [1, 100, 5, 2])[0]) == [0, 6, 0, 0]            # med = element 2 of (1, 2, 5, 100)
