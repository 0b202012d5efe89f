"""tests/mpa_ref.c, the specification of ygz_hip_map_point_attributes, held to two witnesses written another way: a
numpy one -- the rows padded to a dense [P][most rows] table, a loop over the row position, vectorised over the points, the same operation
order -- on every double's bits, and Matcher::PointAttributes' formula restated in plain Python floats on a handful of points."""
import math

import numpy as np

import mpa_ref as mr


def witness(m):
    """the dense-table witness: one pass per row position over all points at once"""
    a = mr.arrays(m)
    c, pw, off = a["center"], a["pw"], a["off"].astype(np.int64)
    P = len(pw)
    rows = off[1:] - off[:-1]
    R = int(rows.max()) if P else 0
    kf = np.zeros((P, max(R, 1)), np.int64)
    for p in range(P):
        kf[p, :rows[p]] = a["kf"][off[p]:off[p + 1]]
    s = np.zeros((P, 3))
    first = np.zeros(P)
    zero = np.zeros(P, bool)
    with np.errstate(all="ignore"):
        for j in range(R):
            on = rows > j
            r = pw - c[kf[:, j]]
            q = r[:, 0] * r[:, 0]
            q = q + r[:, 1] * r[:, 1]
            q = q + r[:, 2] * r[:, 2]
            d = np.sqrt(q)
            zero |= on & (d == 0)
            s[on] = s[on] + (r / d[:, None])[on]
            if j == 0:
                first = d
        has = rows > 0
        lv = np.zeros(P, np.int64)
        lv[has] = np.maximum(a["level"][off[:-1][has]], 0)
        normal = s / np.maximum(rows, 1).astype(np.float64)[:, None]
        dmax = first * (2.0 ** lv)
    fine = np.isfinite(dmax) & np.isfinite(normal).all(axis=1) & ~zero
    state = np.where(has, np.where(fine, 1, 2), 0).astype(np.int32)
    dmax = np.where(state == 1, dmax, 0.0)
    normal = np.where((state == 1)[:, None], normal, 0.0)
    return dict(dmax=dmax, normal=normal, state=state)


def point_attributes(m, p):
    """Matcher::PointAttributes on point p in plain floats: (dmax, normal) or None where its arithmetic gives no finite result"""
    c, pw = np.asarray(m["center"], np.float64), np.asarray(m["pw"], np.float64)
    a, b = int(m["off"][p]), int(m["off"][p + 1])
    if a == b:
        return None
    norm = lambda r: math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    s = [0.0, 0.0, 0.0]
    for e in range(a, b):
        r = [float(pw[p][k]) - float(c[m["kf"][e]][k]) for k in range(3)]
        d = norm(r)
        for k in range(3):
            s[k] += r[k] / d
    r = [float(pw[p][k]) - float(c[m["kf"][a]][k]) for k in range(3)]
    return norm(r) * float(1 << max(int(m["level"][a]), 0)), [v / float(b - a) for v in s]


def test_row_counts_levels_and_repeats_against_the_dense_table():
    rows = [0, 1, 2, 255, 256, 3, 0, 256, 7]
    m = mr.make_map(5, rows, 1)
    m["level"][:] = np.resize(np.array([-1, 0, 7, 30], np.int32), len(m["level"]))
    m["kf"][1:3] = 4                                                      # point 2 sees keyframe 4 twice
    got = mr.attributes(m)
    mr.same(got, witness(m))
    assert got["state"].tolist() == [0, 1, 1, 1, 1, 1, 0, 1, 1]
    assert (got["dmax"][got["state"] == 0] == 0).all() and (got["normal"][got["state"] == 0] == 0).all()
    assert np.abs(np.linalg.norm(got["normal"][got["state"] == 1], axis=1)).max() <= 1 + 1e-12
    # the levels: the first row's, negative ones as 0
    off = m["off"]
    for p, lv in ((1, m["level"][off[1]]), (3, m["level"][off[3]]), (4, m["level"][off[4]])):
        d = np.linalg.norm(m["pw"][p] - m["center"][m["kf"][off[p]]])
        assert abs(got["dmax"][p] / (d * 2.0 ** max(int(lv), 0)) - 1) < 1e-14
    assert {int(m["level"][off[p]]) for p in (1, 2, 3, 4, 5, 7, 8)} == {-1, 0, 7, 30}                # every level stands first somewhere


def test_every_level_on_one_point():
    for lv in (-1, 0, 7, 30):
        m = dict(center=np.array([[0.5, 0.25, -1.0]]), pw=np.array([[1.0, 2.0, 3.0]]), off=np.array([0, 1], np.int32), kf=np.array([0], np.int32),
                 level=np.array([lv], np.int32))
        got = mr.attributes(m)
        mr.same(got, witness(m))
        d = math.sqrt(0.5 * 0.5 + 1.75 * 1.75 + 4.0 * 4.0)
        assert got["state"][0] == 1 and got["dmax"][0] == d * float(1 << max(lv, 0))


def test_larger_random_maps_against_the_dense_table():
    for seed, (K, P) in enumerate([(1, 65), (7, 300), (4096, 257)]):
        m = mr.make_map(K, mr.ragged_rows(P, seed), 10 + seed)
        got = mr.attributes(m)
        mr.same(got, witness(m))
        assert (got["state"] == (np.diff(m["off"]) > 0)).all()


def test_degenerate_points_give_state_2_and_zeros():
    m, states = mr.degenerate_map()
    got = mr.attributes(m)
    mr.same(got, witness(m))
    assert got["state"].tolist() == states
    off = got["state"] != 1
    assert (got["dmax"][off] == 0).all() and (got["normal"][off] == 0).all() and np.isfinite(got["dmax"]).all() and np.isfinite(got["normal"]).all()
    assert not np.signbit(got["dmax"][off]).any() and not np.signbit(got["normal"][off]).any()        # +0.0, not -0.0


def test_point_attributes_formula_in_plain_floats():
    m = mr.make_map(6, [1, 2, 5, 0, 9, 3], 3)
    deg, _ = mr.degenerate_map()
    for mm in (m, deg):
        got = mr.attributes(mm)
        for p in range(len(mm["pw"])):
            if got["state"][p] != 1:
                continue
            dmax, normal = point_attributes(mm, p)
            # Matcher::PointAttributes adds the squares left to right and divides every ray by its norm: the same operations in the same order
            assert got["dmax"][p] == dmax and got["normal"][p].tolist() == normal, p
    assert point_attributes(m, 3) is None and mr.attributes(m)["state"][3] == 0
