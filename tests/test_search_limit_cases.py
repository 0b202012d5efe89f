"""CPU checks of the crafted limit cases of tests/search_limit_cases.py, which tests/test_gpu_search_limits.py runs on k_strack_search (with
the host claim walk) and k_lfuse_search.  For every case three things are shown: the restatement (tests/strack_ref.c, tests/lfuse_ref.c)
gives the case's LITERAL expectation; a numpy witness, written here from the text of DESIGN.md sections 12, 25 and 26 and not from the C
code, gives every output the restatement gives; and the cases DISCRIMINATE: for every wrong variant of a rule (a strict comparison written
as a closed one, a level taken from the wrong place, ...) the witness run with that variant departs from the literals on at least one case
of the rule's row, for every search the rule belongs to.  A variant that no case can tell apart fails the test: the rule would not be
covered.  These are conditions on the cases, not measurements; every comparison is an equality."""
import numpy as np
import pytest

import lfuse_ref as lf
import search_limit_cases as slc
import strack_ref as st

F32 = np.float32
ST_NAMES = ("match", "dist", "level", "reason", "outcome", "n_cand", "n_gated", "proj", "cand", "counts", "rot")
LF_NAMES = ("match", "dist", "pred_level", "reason", "n_gated", "counts")


def restatement(case, sets=None, problems=None, **over):
    mod = st if case.kind == "strack" else lf
    return mod.search(sets or case.sets, problems or case.problems, slc.KX, slc.W, slc.H, case.params["L"], **dict(slc.fields_of(case), **over))


# ---- the witness ---------------------------------------------------------------------------------------------------------------------------
def rotation(q):
    x, y, z, w = (float(a) for a in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def hamming(a, b):
    A, B = np.unpackbits(np.asarray(a, np.uint8), axis=1), np.unpackbits(np.asarray(b, np.uint8), axis=1)
    return (A[:, None, :] != B[None, :, :]).sum(2)


def project(X, R, t, L, local, dmax, normal, v):
    """steps 1-2 of section 26 and, for a point with a distance range, section 12's range, angle and level.  (reason, u, v, iz, pred, c, d)"""
    x, y, z = (np.float64(a) for a in R @ np.asarray(X, np.float64) + t)
    if not (z >= 0 if v == "z_ge" else z > 0):
        return 2, 0, 0, 0, -1, 0, 0
    with np.errstate(all="ignore"):
        iz = np.float64(1) / z
        u, w_ = slc.KX[0] * (x * iz) + slc.KX[2], slc.KX[1] * (y * iz) + slc.KX[3]
    ok_u = (u > 0 if v == "u_open_lower" else u >= 0) and (u <= slc.W if v == "u_closed_upper" else u < slc.W)
    ok_v = (w_ > 0 if v == "v_open_lower" else w_ >= 0) and (w_ <= slc.H if v == "v_closed_upper" else w_ < slc.H)
    if not (ok_u and ok_v):
        return 3, 0, 0, 0, -1, 0, 0
    if not local:
        return 0, u, w_, iz, -1, 0, 0
    d = np.sqrt(x * x + y * y + z * z)
    dmin = dmax / 2.0 ** (L - 1)
    near = d <= 0.8 * dmin if v == "range_lo_le" else d < 0.8 * dmin
    far = d >= 1.2 * dmax if v == "range_hi_ge" else d > 1.2 * dmax
    if near or far:
        return 4, 0, 0, 0, -1, 0, 0
    c = 0.0
    if normal is not None:
        c = float(np.dot((x, y, z), R @ np.asarray(normal, np.float64)))
        if (c <= 0.5 * d if v == "angle_le" else c < 0.5 * d):
            return 5, 0, 0, 0, -1, 0, 0
    ratio = dmax / d
    pred = L - 1
    for m in range(L - 1):                                             # the smallest m with ratio <= 2^m
        if (ratio < 2.0 ** m if v == "level_lt" else ratio <= 2.0 ** m):
            pred = m
            break
    return 0, u, w_, iz, pred, c, d


def in_window(b, u, w_, r, lo, hi, taken, v):
    """steps 5 of section 26 / 7 of section 25: not taken, a level in [lo, hi], |kx - u| < r and |ky - v| < r"""
    px, lv = np.asarray(b["kp_px"], np.float64).reshape(-1, 2), np.asarray(b["kp_level"]).reshape(-1)
    dx, dy = px[:, 0] - u, px[:, 1] - w_
    ok = (np.abs(dx) < r) & (np.abs(dy) < r)
    if v == "win_le_xp":
        ok = (dx <= r) & (dx > -r) & (np.abs(dy) < r)
    elif v == "win_le_xm":
        ok = (dx < r) & (dx >= -r) & (np.abs(dy) < r)
    elif v == "win_le_yp":
        ok = (np.abs(dx) < r) & (dy <= r) & (dy > -r)
    elif v == "win_le_ym":
        ok = (np.abs(dx) < r) & (dy < r) & (dy >= -r)
    return ok & (lv >= lo) & (lv <= hi) & (taken == 0)


def local_range(pred, v):
    return (pred, pred + 1) if v == "local_range_up" else ((pred - 1, pred + 1) if v == "local_range_wide" else (pred - 1, pred))


def is_stereo(kur, v):
    return kur > 0 if v == "stereo_gt0" else kur >= 0


def three_maxima(hist):
    """oracle/bow.c's rule: the three largest bins, an equal count to the earlier bin, an empty bin never"""
    order = [int(b) for b in np.argsort(-np.asarray(hist), kind="stable")[:3] if hist[b] > 0]
    return order + [-1] * (3 - len(order)), [int(hist[b]) for b in order] + [0] * (3 - len(order))


def orientation(pt_angle, kp_angle, match, v):
    """step 9 of section 26 on the matches of the claim walk: (the bin of every match or -1, the histogram, the three maxima)"""
    n = len(match)
    bins, hist = np.full(n, -1), np.zeros(30, int)
    for i in range(n):
        if match[i] < 0:
            continue
        if v == "rot_double":
            rot = np.float64(pt_angle[i]) - np.float64(kp_angle[match[i]])
            rot = rot + 360.0 if rot < 0 else rot
            fb = rot * (1.0 / 30)
        else:
            rot = F32(np.float64(pt_angle[i]) - np.float64(kp_angle[match[i]]))
            rot = F32(rot + F32(360)) if rot < 0 else rot
            fb = np.float64(F32(rot * (F32(1.0) / F32(30))))
        b = int(fb) if v == "rot_trunc" else int(np.floor(fb + 0.5))
        b = 0 if b == 30 else b
        if 0 <= b < 30:
            bins[i] = b
            hist[b] += 1
    ind, mx = three_maxima(hist)
    tenth = np.float64(F32(0.1)) * mx[0] if v == "rot_double" else np.float64(F32(0.1) * F32(mx[0]))
    less = (lambda a: a <= tenth) if v == "rot_tenth_le" else (lambda a: a < tenth)
    if less(mx[1]):
        ind[1] = ind[2] = -1
    elif less(mx[2]):
        ind[2] = -1
    return bins, hist, ind


def witness_strack(case, v=None):
    s, b, prm, L = case.sets[0], case.problems[0], case.params, case.params["L"]
    n, m = slc.n_points(case), slc.n_keypoints(case)
    T = np.asarray(b["T"], np.float64)
    R, t = rotation(T[:4]), T[4:7]
    bf = slc.KX[0] * prm["baseline"]
    local = b["mode"] == slc.LOCAL
    D = hamming(s["pt_desc"], b["kp_desc"])
    taken0 = np.asarray(b["kp_taken"], np.uint8).reshape(-1) if b.get("kp_taken") is not None else np.zeros(m, np.uint8)
    kur = np.asarray(b["kp_ur"], np.float64).reshape(-1) if b.get("kp_ur") is not None else np.full(m, -1.0)
    klv = np.asarray(b["kp_level"]).reshape(-1)
    skip = np.asarray(b["pt_skip"]).reshape(-1) if b.get("pt_skip") is not None else np.zeros(n, np.uint8)
    o = dict(match=np.full(n, -1, np.int32), dist=np.full(n, -1, np.int32), level=np.full(n, -1, np.int32), reason=np.zeros(n, np.int32),
             outcome=np.full(n, -1, np.int32), n_cand=np.zeros(n, np.int32), n_gated=np.zeros(n, np.int32), proj=np.zeros((n, 3)),
             cand=np.full((n, 8), -1, np.int32), counts=np.zeros((1, 4), np.int32), rot=np.zeros((1, 33), np.int32))
    lists = [[] for _ in range(n)]
    for i in range(n):
        if skip[i]:
            o["reason"][i] = 1
            continue
        X = np.asarray(s["pw"], np.float64).reshape(-1, 3)[i]
        why, u, w_, iz, pred, c, d = project(X, R, t, L, local, s["pt_dmax"][i] if local else None, s["pt_normal"][i] if local else None, v)
        o["reason"][i] = why
        if why:
            continue
        ur = u - bf * iz
        if local:
            near = c >= prm["cos_near"] * d if v == "near_ge" else c > prm["cos_near"] * d
            level, r = pred, (b["th"] * (prm["r_near"] if near else prm["r_wide"])) * 2.0 ** pred
            lo, hi = local_range(pred, v)
        else:
            level = int(s["pt_level"][i])
            r = b["th"] * 2.0 ** level
            direction = -b["direction"] if v == "frame_dir_swapped" else b["direction"]
            lo, hi = (level, L - 1) if direction > 0 else ((0, level) if direction < 0 else (level - 1, level + 1))
            if direction == 0 and v == "frame_lo_lvl":
                lo = level
            if direction == 0 and v == "frame_hi_lvl":
                hi = level
        o["level"][i], o["proj"][i] = level, (u, w_, ur)
        win = in_window(b, u, w_, r, lo, hi, taken0, v)
        er = ur - kur
        out = np.abs(er) >= r if v == "gate_ge" else (er > r if v == "gate_upper_only" else (er < -r if v == "gate_lower_only" else np.abs(er) > r))
        out &= is_stereo(kur, v)
        o["n_gated"][i] = int((win & out).sum())
        alive = [int(j) for j in np.nonzero(win & ~out)[0]]
        o["n_cand"][i] = len(alive)
        if v == "first_eight_seen":
            alive = alive[:8]
        lists[i] = sorted(alive, key=lambda j: (D[i, j], -j if v == "sort_ties_larger" else j))[:8]
        o["cand"][i, :len(lists[i])] = lists[i]
    # step 8: the claim walk, points in index order
    taken = taken0.copy()
    for i in range(n):
        if o["reason"][i]:
            continue
        free = [j for j in lists[i] if not taken[j]]
        if not free:
            o["outcome"][i] = 1
            continue
        e1 = free[0]
        d1 = int(D[i, e1])
        if (d1 >= prm["th_dist"] if v == "thdist_ge" else d1 > prm["th_dist"]):
            o["outcome"][i] = 2
            continue
        e2 = free[1] if len(free) > 1 else None
        if v == "e2_next_in_list":
            k = lists[i].index(e1)
            e2 = lists[i][k + 1] if k + 1 < len(lists[i]) else None
        if local and e2 is not None:
            d2 = int(D[i, e2])
            if v == "ratio_float":
                more = F32(d1) > F32(F32(prm["ratio"]) * F32(d2))
            elif v == "ratio_ge":
                more = np.float64(d1) >= prm["ratio"] * np.float64(d2)
            else:
                more = np.float64(d1) > prm["ratio"] * np.float64(d2)
            same = v == "ratio_no_level" or klv[e1] == klv[e2]
            if same and more and not (v == "ratio_e2_within" and d2 > prm["th_dist"]):
                o["outcome"][i] = 3
                continue
        o["outcome"][i], o["match"][i], o["dist"][i], taken[e1] = 0, e1, d1, 1
    o["rot"][0, 30:] = -1
    removed = 0
    if not local and s.get("pt_angle") is not None and prm["check_orientation"]:
        bins, hist, ind = orientation(np.asarray(s["pt_angle"]).reshape(-1), np.asarray(b["kp_angle"]).reshape(-1), o["match"], v)
        o["rot"][0, :30], o["rot"][0, 30:] = hist, ind
        for i in range(n):
            if o["match"][i] >= 0 and (bins[i] < 0 or bins[i] not in ind):
                o["match"][i], o["dist"][i], o["outcome"][i] = -1, -1, 4
                removed += 1
    o["counts"][0] = [(o["match"] >= 0).sum(), (o["reason"] == 0).sum(), (o["n_cand"] > 8).sum(), removed]
    return o


def witness_lfuse(case, v=None):
    s, b, prm, L = case.sets[0], case.problems[0], case.params, case.params["L"]
    n, m = slc.n_points(case), slc.n_keypoints(case)
    T = np.asarray(b["T"], np.float64)
    R, t = rotation(T[:4]), T[4:7]
    bf = slc.KX[0] * prm["baseline"]
    D = hamming(s["pt_desc"], b["kp_desc"])
    taken = np.asarray(b["kp_taken"], np.uint8).reshape(-1) if b.get("kp_taken") is not None else np.zeros(m, np.uint8)
    kur = np.asarray(b["kp_ur"], np.float64).reshape(-1) if b.get("kp_ur") is not None else np.full(m, -1.0)
    px, klv = np.asarray(b["kp_px"], np.float64).reshape(-1, 2), np.asarray(b["kp_level"]).reshape(-1)
    skip = np.asarray(b["pt_skip"]).reshape(-1) if b.get("pt_skip") is not None else np.zeros(n, np.uint8)
    o = dict(match=np.full(n, -1, np.int32), dist=np.full(n, -1, np.int32), pred_level=np.full(n, -1, np.int32), reason=np.zeros(n, np.int32),
             n_gated=np.zeros(n, np.int32), counts=np.zeros((1, 2), np.int32))
    for i in range(n):
        if skip[i]:
            o["reason"][i] = 1
            continue
        X = np.asarray(s["pw"], np.float64).reshape(-1, 3)[i]
        why, u, w_, iz, pred, c, d = project(X, R, t, L, True, s["pt_dmax"][i], s["pt_normal"][i] if s.get("pt_normal") is not None else None, v)
        o["reason"][i] = why
        if why:
            continue
        o["pred_level"][i] = pred
        ur = u - bf * iz
        lo, hi = local_range(pred, v)
        win = in_window(b, u, w_, prm["th"] * 2.0 ** pred, lo, hi, taken, v)
        ex, ey, er = u - px[:, 0], w_ - px[:, 1], ur - kur
        stereo = is_stereo(kur, v)
        e2 = np.where(stereo, ex * ex + ey * ey + er * er, ex * ex + ey * ey)
        s2 = 4.0 ** (pred if v == "chi_pred_level" else klv)
        chi2 = np.where(stereo & (v != "chi_mono_on_stereo"), prm["chi2_stereo"], prm["chi2_mono"])
        out = e2 >= chi2 * s2 if v == "chi_ge" else e2 > chi2 * s2
        o["n_gated"][i] = int((win & out).sum())
        alive = [int(j) for j in np.nonzero(win & ~out)[0]]
        if alive:
            j = min(alive, key=lambda j: (D[i, j], j))
            if (D[i, j] < prm["th_dist"] if v == "dist_lt" else D[i, j] <= prm["th_dist"]):
                o["match"][i], o["dist"][i] = j, D[i, j]
    o["counts"][0] = [(o["match"] >= 0).sum(), (o["reason"] == 0).sum()]
    return o


def witness(case, v=None):
    return witness_strack(case, v) if case.kind == "strack" else witness_lfuse(case, v)


def same(a, b, names):
    return [k for k in names if not (np.asarray(a[k]).shape == np.asarray(b[k]).shape and np.array_equal(np.asarray(a[k]), np.asarray(b[k])))]


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
ROWS = {"z>0", "image bounds", "distance range", "viewing angle", "predicted level", "radius factor", "frame level range", "local level range",
        "window", "right-column gate", "stereo iff kp_ur >= 0", "chi-square gate", "lfuse th_dist", "sorted list", "th_dist", "ratio", "claim",
        "orientation"}
ALL3, LOCAL2 = ("lfuse", "local", "frame"), ("lfuse", "local")
VARIANTS = [(v, tag, row) for row, tags, vs in (
    ("z>0", ALL3, ("z_ge",)),
    ("image bounds", ALL3, ("u_closed_upper", "u_open_lower", "v_closed_upper", "v_open_lower")),
    ("distance range", LOCAL2, ("range_hi_ge", "range_lo_le")),
    ("viewing angle", LOCAL2, ("angle_le",)),
    ("predicted level", LOCAL2, ("level_lt",)),
    ("radius factor", ("local",), ("near_ge",)),
    ("frame level range", ("frame",), ("frame_lo_lvl", "frame_hi_lvl", "frame_dir_swapped")),
    ("local level range", LOCAL2, ("local_range_up", "local_range_wide")),
    ("window", ALL3, ("win_le_xp", "win_le_xm", "win_le_yp", "win_le_ym")),
    ("right-column gate", ("frame", "local"), ("gate_ge", "gate_upper_only", "gate_lower_only")),
    ("stereo iff kp_ur >= 0", ALL3, ("stereo_gt0",)),
    ("chi-square gate", ("lfuse",), ("chi_ge", "chi_pred_level", "chi_mono_on_stereo")),
    ("lfuse th_dist", ("lfuse",), ("dist_lt",)),
    ("sorted list", ("frame",), ("sort_ties_larger", "first_eight_seen")),
    ("th_dist", ("frame", "local"), ("thdist_ge",)),
    ("ratio", ("local",), ("ratio_ge", "ratio_float", "ratio_no_level", "ratio_e2_within")),
    ("claim", ("local",), ("e2_next_in_list",)),
    ("orientation", ("frame",), ("rot_trunc", "rot_tenth_le", "rot_double")),
) for tag in tags for v in vs]


def tag(case):
    return case.name.split("/")[0]


def test_every_row_has_cases_with_literals_and_every_case_is_run():
    base, every = slc.base_cases(), slc.all_cases()
    assert {c.row for c in base} == ROWS and all(c.expected for c in base)
    assert len(every) == len(base) * (1 + len(slc.KP_POSITIONS) + len(slc.PT_POSITIONS))           # nothing is left out
    for c in every:
        if "@kp" in c.name:
            assert slc.n_keypoints(c) == slc.N_EMBED
        if "@pt" in c.name:
            assert slc.n_points(c) == slc.N_EMBED and 1 <= int((np.asarray(c.problems[0]["pt_skip"]) == 0).sum()) <= 32
        assert slc.n_points(c) <= 257 and slc.n_keypoints(c) <= 257
    # the decisive keypoints land where the sweep changes its path: both sides of a group of eight and of a tile of 256, the ragged end
    two = next(c for c in base if c.name == "frame/a tie of two")
    assert [slc.keypoints_at(two, p).expected["cand"][0][:2] for p in slc.KP_POSITIONS] == [[0, 1], [7, 8], [8, 9], [255, 256], [255, 256]]


def test_the_ratio_limits_are_equalities_in_fp64():
    for k in range(1, 52):
        assert 0.8 * np.float64(5 * k) == np.float64(4 * k) and 0.6 * np.float64(5 * k) == np.float64(3 * k), k
    assert slc.down(0.8) * 5.0 < 4.0 and F32(slc.down(0.8)) * F32(5) == F32(4)
    assert 1.2 * 5.0 == 6.0 and 0.8 * (5.0 / 4) == 1.0


def test_restatement_gives_the_literals_and_the_witness_agrees():
    for c in slc.all_cases():
        ref = restatement(c)
        assert slc.holds(c, ref) == [], c.name
        wit = witness(c)
        assert same(wit, ref, ST_NAMES if c.kind == "strack" else LF_NAMES) == [], c.name
        assert slc.holds(c, wit) == [], c.name


@pytest.mark.parametrize("variant,kind,row", VARIANTS)
def test_the_cases_separate_the_wrong_variant(variant, kind, row):
    cases = [c for c in slc.base_cases() if c.row == row and tag(c) == kind]
    assert cases
    told = [c.name for c in cases if slc.holds(c, witness(c, variant))]
    assert told, "no case of %r tells %s apart on %s" % (row, variant, kind)


def test_every_variant_of_the_witness_is_in_the_table():
    import inspect
    import re
    src = "".join(inspect.getsource(f) for f in (project, in_window, local_range, is_stereo, orientation, witness_strack, witness_lfuse))
    assert set(re.findall(r'v [!=]= "(\w+)"', src)) == {v for v, _, _ in VARIANTS}


def test_orientation_cases_are_the_oracles(oracle):
    cases = [c for c in slc.base_cases() if c.row == "orientation"]
    assert len(cases) >= 15
    for c in cases:
        on, off = restatement(c), restatement(c, check_orientation=0)
        cnt, hist, ind = oracle.bow_orientation(c.sets[0]["pt_angle"], c.problems[0]["kp_angle"], off["match"])
        assert cnt == on["counts"][0, 0] and list(on["rot"][0, :30]) == list(hist) and list(on["rot"][0, 30:]) == list(ind), c.name
        assert on["counts"][0, 3] == off["counts"][0, 0] - cnt


def test_packed_calls_hold_every_case_where_it_says():
    every = slc.all_cases()
    seen = 0
    for fam in slc.families(every):
        for sets, problems, slots in slc.pack(fam):
            assert 1 <= len(problems) <= 64 and len(sets) <= 8 and all(len(s["pt_desc"]) <= 257 for s in sets)
            c0 = slots[0][0]
            out = restatement(c0, sets, problems)
            offs = (st if c0.kind == "strack" else lf).offsets(sets, problems)
            for slot in slots:
                assert slc.holds(slot[0], slc.slot_outputs(out, offs, slot)) == [], slot[0].name
                seen += 1
            live = np.zeros(int(offs[-1]), bool)                      # every point outside the cases' slots is skipped
            for c, q, at, n in slots:
                live[int(offs[q]) + at:int(offs[q]) + at + n] = True
            assert (out["reason"][~live] == 1).all()
    assert seen == len(every)
    assert max(len(p) for fam in slc.families(every) for _, p, _ in slc.pack(fam)) == 64             # blockIdx.y up to 63 is reached
