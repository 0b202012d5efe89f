"""CPU checks of the crafted limit cases of tests/depth_limit_cases.py, which tests/test_gpu_depth_limits.py runs on k_smap_pairs and on
k_stereo_match / k_stereo_median.  For every case three things are shown: the restatement (tests/smap_ref.c, tests/stereo_ref.c) gives the
case's LITERAL expectation; a numpy witness, written here from the text of DESIGN.md sections 19 and 24 and not from the C code, gives every
output the restatement gives (the position of a triangulated point excepted: the witness takes its null vector from np.linalg.svd, so
every case that asks about a later step un-projects); and the cases DISCRIMINATE: for every wrong variant of a rule (a strict comparison
written as a closed one, a level or a radius taken from the wrong side, ...) the witness run with that variant departs from the literals on
at least one case of the rule's row.  A variant that no case can tell apart fails the test: the rule would not be covered.  No pair is
marked or skipped, and every comparison is an equality."""
import numpy as np
import pytest

import depth_limit_cases as dlc
import smap_ref as sm
import stereo_ref as sr


# ==== map-point pairs ===========================================================================================================================
def restate_pairs(case, pb=None):
    return sm.create(pb if pb is not None else case.pb, case.K4, sm.default_params(**case.params))


def rotation(q):
    x, y, z, w = (float(a) for a in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def mv(M, a):
    """M a, every sum left to right (section 24: "every sum left to right")"""
    return (M[:, 0] * a[0] + M[:, 1] * a[1]) + M[:, 2] * a[2]


def witness_pair(pb, i, K4, prm, v=None):
    """section 24 (a), steps 1-8, for pair i of a problem: (code, method, pos_world)"""
    fx, fy, cx, cy = K4
    b, bf = prm["baseline"], K4[0] * prm["baseline"]
    T1, T2 = np.asarray(pb["T1"], np.float64), np.asarray(pb["T2"], np.float64)
    R1, R2, t1, t2 = rotation(T1[:4]), rotation(T2[:4]), T1[4:], T2[4:]
    px = [np.asarray(pb["px1"], np.float64).reshape(-1, 2)[i], np.asarray(pb["px2"], np.float64).reshape(-1, 2)[i]]
    ur = [float(np.asarray(pb["ur1"]).reshape(-1)[i]), float(np.asarray(pb["ur2"]).reshape(-1)[i])]
    lvl = [int(np.asarray(pb["level1"]).reshape(-1)[i]), int(np.asarray(pb["level2"]).reshape(-1)[i])]
    stereo = [u > 0 if v == "stereo_gt0" else u >= 0 for u in ur]
    d = [float(np.asarray(pb["depth%d" % (k + 1)]).reshape(-1)[i]) if stereo[k] else None for k in range(2)]      # a mono side's depth is not read
    none = (0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        xn = [np.array([(p[0] - cx) / fx, (p[1] - cy) / fy, 1.0]) for p in px]
        ray = [mv(R1.T, xn[0]), mv(R2.T, xn[1])]
        norm = [np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) for r in ray]
        cos_rays = float(((ray[0][0] * ray[1][0] + ray[0][1] * ray[1][1]) + ray[0][2] * ray[1][2]) / (norm[0] * norm[1]))
        closed = lambda z: (z * z - (b / 2) * (b / 2)) / (z * z + (b / 2) * (b / 2))
        cs = [cos_rays + 1.0, cos_rays + 1.0]
        if stereo[0]:
            cs[0] = closed(d[0])
        if stereo[1] and (not stereo[0] or v == "cosS2_always"):
            cs[1] = closed(d[1])
        cos_s = min(cs)
        below = cos_rays <= cos_s if v == "cosrays_le_cosS" else cos_rays < cos_s
        positive = cos_rays >= 0 if v == "cosrays_ge0" else cos_rays > 0
        free = (stereo[0] or stereo[1]) and v != "parallax_on_stereo"
        gate = free or (cos_rays <= prm["cos_parallax_max"] if v == "parallax_le" else cos_rays < prm["cos_parallax_max"])
        less = (lambda p, q: p <= q) if v == "tie_le" else (lambda p, q: p < q)
        if below and positive and gate:
            method = 1
            P1, P2 = np.hstack([R1, t1[:, None]]), np.hstack([R2, t2[:, None]])
            A = np.stack([xn[0][0] * P1[2] - P1[0], xn[0][1] * P1[2] - P1[1], xn[1][0] * P2[2] - P2[0], xn[1][1] * P2[2] - P2[1]])
            x = np.linalg.svd(A)[2][3]
            if abs(x[3]) < 1e-300 or not np.all(np.isfinite(x[:3] / x[3])):
                return 2, method, none
            X = x[:3] / x[3]
        elif stereo[0] and less(cs[0], cs[1]):
            method, X = 2, mv(R1.T, d[0] * xn[0] - t1)
        elif stereo[1] and less(cs[1], cs[0]):
            method, X = 3, mv(R2.T, d[1] * xn[1] - t2)
        else:
            return 1, 0, none
        Pc = [mv(R1, X) + t1, mv(R2, X) + t2]
        closed_at_0 = (v == "z1_ge", v == "z2_ge")
        for k in ((1, 0) if v == "z2_first" else (0, 1)):
            if not (Pc[k][2] >= 0 if closed_at_0[k] else Pc[k][2] > 0):
                return 3 + k, method, none

        def refused(k):
            u, w_ = fx * (Pc[k][0] / Pc[k][2]) + cx, fy * (Pc[k][1] / Pc[k][2]) + cy
            e2 = (u - px[k][0]) ** 2 + (w_ - px[k][1]) ** 2
            chi2, closed_gate = prm["chi2_mono"], v == "chi_mono_ge"
            if stereo[k]:
                e2 = e2 + ((u - bf / Pc[k][2]) - ur[k]) ** 2
                chi2, closed_gate = prm["chi2_mono"] if v == "chi_mono_on_stereo" else prm["chi2_stereo"], v == "chi_stereo_ge"
            th = chi2 * 4.0 ** lvl[1 - k if v == "chi_other_level" else k]
            return e2 >= th if closed_gate else e2 > th
        for k in ((1, 0) if v == "code6_first" else (0, 1)):
            if refused(k):
                return 5 + k, method, none
        O = [-mv(R1.T, t1), -mv(R2.T, t2)]
        dist = [float(np.sqrt(((X - o) ** 2).sum())) for o in O]
        if dist[0] == 0 or dist[1] == 0:
            return 7, method, none
        rd, ro, f = dist[1] / dist[0], 2.0 ** lvl[0] / 2.0 ** lvl[1], prm["ratio_factor"]
        low = rd * f <= ro if v == "scale_lo_le" else rd * f < ro
        high = rd >= ro * f if v == "scale_hi_ge" else rd > ro * f
        if low or high:
            return 8, method, none
    return 0, method, tuple(float(a) for a in X)


PAIR_VARIANTS = [(v, row) for row, vs in (
    ("ur", ("stereo_gt0",)),
    ("cosRays==cosS", ("cosrays_le_cosS",)),
    ("cosRays==0", ("cosrays_ge0",)),
    ("cos_parallax_max", ("parallax_le", "parallax_on_stereo")),
    ("asymmetry", ("cosS2_always", "tie_le")),
    ("z>0", ("z1_ge", "z2_ge", "z2_first")),
    ("reprojection", ("chi_mono_ge", "chi_stereo_ge", "chi_other_level", "chi_mono_on_stereo", "code6_first", "stereo_gt0")),
    ("scale", ("scale_lo_le", "scale_hi_ge")),
) for v in vs]


def test_every_pair_row_has_cases_on_and_off_its_limit():
    cases = dlc.pair_cases()
    assert {c.row for c in cases} == set(dlc.PAIR_ROWS) and len(cases) == 70
    for row in dlc.PAIR_ROWS[:-1]:
        names = [c.name for c in cases if c.row == row]
        assert any("on" in n.split("/")[-1].split() or "=" in n or "tie" in n for n in names), row
        assert any("step" in n or "below" in n or "above" in n for n in names), row
    assert {c.expected[0] for c in cases} == set(range(9))                     # every code is some case's literal


def test_pair_restatement_gives_the_literals_and_the_witness_agrees():
    for c in dlc.pair_cases():
        code, method, pos = restate_pairs(c)
        assert dlc.pair_holds(c, code[0], method[0], pos[0]) == [], c.name
        w = witness_pair(c.pb, 0, c.K4, c.params)
        assert (w[0], w[1]) == (code[0], method[0]), c.name
        assert dlc.pair_holds(c, *w) == [], c.name
        if method[0] != 1:                                                  # an un-projected point is the same double, bit for bit
            assert dlc.equal_bits(pos[0], w[2]), c.name


@pytest.mark.parametrize("variant,row", PAIR_VARIANTS)
def test_the_pair_cases_separate_the_wrong_variant(variant, row):
    cases = [c for c in dlc.pair_cases() if c.row == row]
    told = [c.name for c in cases if dlc.pair_holds(c, *witness_pair(c.pb, 0, c.K4, c.params, variant))]
    assert told, "no case of %r tells %s apart" % (row, variant)


def test_pairs_embedded_in_257_pairs():
    for c in dlc.pair_cases():
        f, f_code = dlc.filler(c)
        assert f_code != c.expected[0]
        for pos in dlc.PAIR_POSITIONS:
            pb = dlc.pair_at(c, pos)
            code, method, xyz = restate_pairs(c, pb)
            assert len(code) == dlc.N_EMBED and dlc.pair_holds(c, code[pos], method[pos], xyz[pos]) == [], (c.name, pos)
            others = np.arange(dlc.N_EMBED) != pos
            assert (code[others] == f_code).all() and not xyz[others].any(), (c.name, pos)
            assert witness_pair(pb, pos, c.K4, c.params)[:2] == (code[pos], method[pos])
            assert witness_pair(pb, (pos + 1) % dlc.N_EMBED, c.K4, c.params)[0] == f_code


def test_pairs_as_one_problem_of_32():
    for c in dlc.pair_cases():
        # reading a neighbour's cameras would change the literal
        other = dict(c.pb, T1=np.array(dlc.NEIGHBOUR_T1), T2=np.array(dlc.NEIGHBOUR_T2))
        code, method, xyz = restate_pairs(c, other)
        assert dlc.pair_holds(c, code[0], method[0], xyz[0]) != [], c.name
        for pos in dlc.PROBLEM_POSITIONS:
            pbs = dlc.problems_around(c, pos)
            assert len(pbs) == dlc.N_PROBLEMS and pbs[pos] is c.pb and sum(p["n"] == 0 for p in pbs) >= 8
            assert all(pbs[q]["n"] == 0 for q in (pos - 1, pos + 1) if 0 <= q < dlc.N_PROBLEMS)
            assert all(not np.array_equal(p["T1"], c.pb["T1"]) and not np.array_equal(p["T2"], c.pb["T2"]) for q, p in enumerate(pbs) if q != pos)


# ==== stereo depths =============================================================================================================================
@pytest.fixture(scope="module")
def levels(oracle):
    """name -> the three levels of each picture, built once"""
    return {name: oracle.pyramid(img, dlc.LEVELS) for name, img in dlc.pictures().items()}


def restate_depths(case, levels):
    return sr.match(levels["zero"], levels[case.right], case.kl, case.kr, sr.params(**case.params), fx=dlc.FX)


def witness_depths(case, levels, v=None):
    """section 19, steps 1-10 and the median rule"""
    left, right, kl, kr, p = levels["zero"], levels[case.right], case.kl, case.kr, case.params
    nl = len(kl["level"])
    bf, mind, maxd = dlc.FX * p["baseline"], p["min_disparity"], (p["max_disparity"] if p["max_disparity"] != 0.0 else dlc.FX)
    o = dict(right_idx=np.full(nl, -1, np.int32), u_right=np.full(nl, -1.0), depth=np.full(nl, -1.0), sad=np.full(nl, -1, np.int32),
             status=np.full(nl, sr.NO_CANDIDATE, np.int32), best_idx=np.full(nl, -1, np.int32), best_dist=np.full(nl, -1, np.int32),
             n_cand=np.zeros(nl, np.int32), sads=np.full((nl, 11), -1, np.int32))
    ur, vr, lr = kr["px"][:, 0], kr["px"][:, 1], kr["level"].astype(np.int64)
    bits_l, bits_r = np.unpackbits(kl["desc"], axis=1), np.unpackbits(kr["desc"], axis=1)
    half = [0.0 if v == name else 0.5 for name in ("no_half_su", "no_half_sv", "no_half_sr")]
    for i in range(nl):
        ul, vl, l = float(kl["px"][i, 0]), float(kl["px"][i, 1]), int(kl["level"][i])
        if (ul - mind <= 0 if v == "step1_le" else ul - mind < 0):
            continue
        band = 2.0 * np.exp2(l if v == "r_from_left_level" else lr)
        top, bottom, row = np.floor(vr - band), np.ceil(vr + band), np.floor(vl)
        gap = np.abs(lr - l)
        ok = gap < 1 if v == "level_lt1" else (gap <= 2 if v == "level_le2" else gap <= 1)
        ok = ok & (top < row if v == "band_top_lt" else top <= row) & (row < bottom if v == "band_bottom_lt" else row <= bottom)
        ok = ok & (ur > ul - maxd if v == "col_lo_gt" else ur >= ul - maxd) & (ur < ul - mind if v == "col_hi_lt" else ur <= ul - mind)
        cand = np.nonzero(ok)[0]
        o["n_cand"][i] = len(cand)
        if not len(cand):
            continue
        dist = (bits_r[cand] != bits_l[i]).sum(axis=1)
        j, dj = min(zip(cand, dist), key=lambda e: (e[1], -e[0] if v == "tie_largest_j" else e[0]))
        o["best_idx"][i], o["best_dist"][i] = j, dj
        if (dj > p["th_dist"] if v == "thdist_gt" else dj >= p["th_dist"]):
            o["status"][i] = sr.DESCRIPTOR
            continue
        s = float(2 ** l)
        su, sv, sc = int(np.floor(ul / s + half[0])), int(np.floor(vl / s + half[1])), int(np.floor(float(ur[j]) / s + half[2]))
        il, ir = left[l].astype(np.int64), right[l].astype(np.int64)
        hl, wl = il.shape
        inside = (5 <= su) and (su <= wl - 5 if v == "su_hi_le" else su < wl - 5)
        inside = inside and (5 < sv if v == "sv_lo_lt" else 5 <= sv) and (sv <= hl - 5 if v == "sv_hi_le" else sv < hl - 5)
        inside = inside and (sc - 10 > 0 if v == "sr_lo_gt" else sc - 10 >= 0) and (sc + 10 <= wl if v == "sr_hi_le" else sc + 10 < wl)
        if not inside:
            o["status"][i] = sr.BORDER
            continue
        il, ir, su, sv, sc = np.pad(il, 16), np.pad(ir, 16), su + 16, sv + 16, sc + 16          # a variant's window may leave the picture: zeros there
        a = il[sv - 5:sv + 6, su - 5:su + 6] - il[sv, su]
        D = np.array([np.abs(a - (ir[sv - 5:sv + 6, sc + inc - 5:sc + inc + 6] - ir[sv, sc + inc])).sum() for inc in range(-5, 6)])
        sc -= 16
        o["sads"][i] = D
        q = int(np.nonzero(D == D.min())[0][-1 if v == "last_minimum" else 0])
        if (q <= 1 or q >= 9) if v == "edge_wide" else (q == 0 or q == 10):
            o["status"][i] = sr.EDGE
            continue
        d1, d2, d3 = int(D[q - 1]), int(D[q]), int(D[q + 1])
        with np.errstate(all="ignore"):
            delta = np.float64(d3 - d1 if v == "delta_sign" else d1 - d3) / np.float64(2 * (d1 + d3 - 2 * d2))
            urs = s * (float(sc + q - 5) + delta)
            disp = ul - urs
            if not ((mind < disp if v == "disp_gt_minD" else mind <= disp) and (disp <= maxd if v == "disp_le_maxD" else disp < maxd)):
                o["status"][i] = sr.DISPARITY
                continue
            if (disp < 0 if v == "disp_lt0_branch" else disp <= 0):
                disp, urs = 0.01, ul - 0.01
            o["status"][i], o["right_idx"][i], o["u_right"][i], o["depth"][i], o["sad"][i] = sr.OK, j, urs, bf / disp, d2
    ok = o["status"] == sr.OK
    if ok.any():
        m = int(ok.sum())
        med = int(np.sort(o["sad"][ok])[(m - 1) // 2 if v == "median_lower" else m // 2])
        sad = o["sad"].astype(np.int64)
        lost = ok & (10 * sad >= 21 * med if v == "median_ge" else 10 * sad > 21 * med)
        o["status"][lost], o["u_right"][lost], o["depth"][lost] = sr.MEDIAN, -1.0, -1.0
    o["counts"] = np.bincount(o["status"], minlength=7).astype(np.int32)
    return o


DEPTH_VARIANTS = [(v, row) for row, vs in (
    ("uL-minD", ("step1_le",)),
    ("level gate", ("level_lt1", "level_le2")),
    ("row band", ("band_top_lt", "band_bottom_lt", "r_from_left_level")),
    ("column range", ("col_lo_gt", "col_hi_lt")),
    ("th_dist", ("thdist_gt",)),
    ("tie to the smallest j", ("tie_largest_j",)),
    ("rounding", ("no_half_su", "no_half_sv", "no_half_sr")),
    ("border", ("su_hi_le", "sv_lo_lt", "sv_hi_le", "sr_lo_gt", "sr_hi_le")),
    ("k=+-L", ("edge_wide", "last_minimum")),
    ("delta", ("delta_sign",)),
    ("disparity", ("disp_gt_minD", "disp_le_maxD", "disp_lt0_branch")),
    ("median", ("median_lower", "median_ge")),
) for v in vs]
ALL_FIELDS = sr.OUTPUTS + sr.STAGES


def test_every_depth_row_has_cases_with_literals():
    cases = dlc.depth_cases()
    assert {c.row for c in cases} == set(dlc.DEPTH_ROWS) and len(cases) == 138 and all(c.expected for c in cases)
    assert {s for c in cases for s in c.expected["status"]} == set(range(7))         # every status is some case's literal
    assert max(len(c.kl["level"]) for c in cases) == 390 and max(len(c.kr["level"]) for c in cases) == 257


def test_the_designed_pictures_give_the_designed_columns(levels):
    """strip by strip: the eleven sums of section 19's step 6 on the designed pictures are the columns the cases were written from"""
    zero = levels["zero"]
    for name, D in dlc.STRIPS.items():
        sr_, sv = dlc.strip_at(name)
        ir = levels["level0"][0].astype(np.int64)
        got = [int(np.abs(ir[sv - 5:sv + 6, sr_ + q - 10:sr_ + q + 1] - ir[sv, sr_ + q - 5]).sum()) for q in range(11)]
        assert got == D and not zero[0].any(), name
    for name, (sv, _, D, _) in dlc.BLOBS.items():
        ir = levels["level1"][1].astype(np.int64)
        got = [int(np.abs(ir[sv - 5:sv + 6, dlc.BLOB_SR + q - 10:dlc.BLOB_SR + q + 1] - ir[sv, dlc.BLOB_SR + q - 5]).sum()) for q in range(11)]
        assert got == D, name


def test_depth_restatement_gives_the_literals_and_the_witnesses_agree(levels):
    for c in dlc.depth_cases():
        ref = restate_depths(c, levels)
        assert dlc.depth_holds(c, ref) == [], c.name
        wit = witness_depths(c, levels)
        other = sr.witness(levels["zero"], levels[c.right], c.kl, c.kr, sr.params(**c.params), fx=dlc.FX)      # the witness the scenes are held to
        for k in ALL_FIELDS:
            assert dlc.equal_bits(ref[k], wit[k]) and dlc.equal_bits(ref[k], other[k]), (c.name, k)
        assert dlc.depth_holds(c, wit) == [], c.name


@pytest.mark.parametrize("variant,row", DEPTH_VARIANTS)
def test_the_depth_cases_separate_the_wrong_variant(levels, variant, row):
    cases = [c for c in dlc.depth_cases() if c.row == row]
    told = [c.name for c in cases if dlc.depth_holds(c, witness_depths(c, levels, variant))]
    assert told, "no case of %r tells %s apart" % (row, variant)


def test_every_variant_of_the_witnesses_is_in_the_tables():
    import inspect
    import re
    for fn, table in ((witness_pair, PAIR_VARIANTS), (witness_depths, DEPTH_VARIANTS)):
        src = inspect.getsource(fn)
        assert set(re.findall(r'v [!=]= "(\w+)"', src)) | set(re.findall(r'"(no_half_\w+)"', src)) == {v for v, _ in table}
