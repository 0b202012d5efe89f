"""The specification of ygz_hip_stereo_local_map_resident as a composition of frozen parts: tests/lms_ref.py (the
selection), tests/mpa_ref.py (the attributes) and tests/slm_ref.py (the tracking), joined by the filter that this file restates in plain
Python loops (steps 2 to 4 of the header: the refused points, the compaction with `moved`, the prior rows).  Nothing here runs on a device.

A `world` is a dict: K, kf_bad [K], C, cov [K, C], off [P + 1], kf, feat [n_obs], pt_bad [P] or None (the selection side, as a case of
lms_ref); center [Kc, 3], a_off [P + 1], a_kf, a_level (the attribute side, as a map of mpa_ref with pw); pw [P, 3], pt_desc [P, 32],
pt_has_desc [P] or None."""
import numpy as np

import lms_ref
import mpa_ref
import slm_ref

FILL = -7                                                               # what an output entry nobody wrote holds
PER_POINT = slm_ref.INT_OUTPUTS + ("proj",)
SELECT = ("votes", "ref", "n_voters", "n_local", "local_kf", "n_cut", "n_pt", "local_pt", "n_removed", "prior")


def refused(state, has_desc):
    """step 2: point p is refused when state[p] != 1 or pt_has_desc[p] == 0"""
    out = []
    for p in range(len(state)):
        out.append(1 if (int(state[p]) != 1 or (has_desc is not None and int(has_desc[p]) == 0)) else 0)
    return np.array(out, np.uint8)


def filter_lists(local_pt, n_pt, ref):
    """step 3 on local_pt [F, MP] and n_pt [F] of the selection: (local_pt after the filter, padded with -1; n_pt; n_removed; moved, a list
    of one array per frame with the new position of every entry, or -1)"""
    local_pt = np.asarray(local_pt, np.int32)
    F, MP = local_pt.shape
    out, n_out, n_rem, moved = np.full((F, MP), -1, np.int32), [], [], []
    for f in range(F):
        m, mv = 0, []
        for i in range(int(n_pt[f])):
            p = int(local_pt[f, i])
            if ref[p]:
                mv.append(-1)
                continue
            mv.append(m)
            out[f, m] = p
            m += 1
        n_out.append(m)
        n_rem.append(int(n_pt[f]) - m)
        moved.append(np.array(mv, np.int32))
    return out, np.array(n_out, np.int32), np.array(n_rem, np.int32), moved


def prior_rows(fr_off, fr_prior, moved, cells):
    """step 4: prior[f][j] = moved[f][fr_prior[fr_off[f] + j]] for an entry j of frame f with a position in the selected list, else -1"""
    F = len(fr_off) - 1
    out = np.full((F, cells), -1, np.int32)
    for f in range(F):
        n = int(fr_off[f + 1]) - int(fr_off[f])
        assert n <= cells
        for j in range(n):
            at = int(fr_prior[int(fr_off[f]) + j])
            if 0 <= at < len(moved[f]):
                out[f, j] = moved[f][at]
    return out


def strided(o, n_pt, MP, fill=FILL):
    """the per-point outputs of a call that concatenates them (slm_ref, the indexed call), laid out [F, MP]: row f holds n_pt[f] entries"""
    F = len(n_pt)
    off = np.concatenate([[0], np.cumsum(n_pt)]).astype(np.int64)
    out = {k: v for k, v in o.items() if k not in PER_POINT and k != "offsets"}
    for k in PER_POINT:
        v = np.asarray(o[k])
        a = np.full((F, MP) + v.shape[1:], fill, v.dtype)
        for f in range(F):
            a[f, :int(n_pt[f])] = v[off[f]:off[f + 1]]
        out[k] = a
    return out


def select_case(world, fr_off, fr_pt, lms):
    return dict(K=world["K"], kf_bad=world["kf_bad"], C=world["C"], cov=world["cov"], off=world["off"], kf=world["kf"], feat=world["feat"],
                pt_bad=world["pt_bad"], fr_off=np.asarray(fr_off, np.int32), fr_pt=np.asarray(fr_pt, np.int32), params=dict(lms))


def attribute_map(world):
    return dict(center=world["center"], pw=world["pw"], off=world["a_off"], kf=world["a_kf"], level=world["a_level"])


def join(sel, attr, world, fr_off, cells, track):
    """steps 2 to 5 behind a selection `sel` and attributes `attr`, wherever they were computed; track(points, lists, prior rows) runs step 5 and
    returns its outputs with the per-point ones concatenated.  The outputs of the resident call"""
    ref = refused(attr["state"], world["pt_has_desc"])
    MP = sel["local_pt"].shape[1]
    lp, n_pt, n_rem, moved = filter_lists(sel["local_pt"], sel["n_pt"], ref)
    prior = prior_rows(fr_off, sel["fr_prior"], moved, cells)
    points = dict(pw=world["pw"], pt_desc=world["pt_desc"], pt_dmax=attr["dmax"], pt_normal=attr["normal"])
    out = strided(track(points, [lp[f, :n_pt[f]].tolist() for f in range(len(n_pt))], prior), n_pt, MP)
    out.update({k: sel[k] for k in ("votes", "ref", "n_voters", "n_local", "local_kf", "n_cut")})
    out.update(n_pt=n_pt, local_pt=lp, n_removed=n_rem, prior=prior)
    return out


def resident(world, frames, slots, T, fr_off, fr_pt, cells, lms=None, **kw):
    """the whole call on the host: frames maps a slot to its arrays as slm_ref wants them; kw goes to slm_ref.local_map (K, w, h, L and the
    fields of ygz_slm_params)"""
    sel = lms_ref.select(select_case(world, fr_off, fr_pt, lms or {}))
    attr = mpa_ref.attributes(attribute_map(world))

    def track(points, lists, prior):
        sets = [{k: np.asarray(points[k])[np.asarray(l, np.int64)] for k in points} if len(l) else dict() for l in lists]
        pr = [prior[f, :len(np.asarray(frames[int(s)]["level"]).reshape(-1))] for f, s in enumerate(slots)]
        return slm_ref.local_map(frames, sets, slots, list(range(len(slots))), T, pr, cells=cells, **kw)
    return join(sel, attr, world, fr_off, cells, track)


def map_arrays(world):
    """the fields of ygz_map_arrays of a world"""
    return dict(kf_bad=world["kf_bad"], cov=world["cov"], n_cov=world["C"], offsets=world["off"], kf=world["kf"], feat=world["feat"],
                pt_bad=world["pt_bad"], centre=world["center"], a_offsets=world["a_off"], a_kf=world["a_kf"], a_level=world["a_level"],
                pw=world["pw"], pt_desc=world["pt_desc"], pt_has_desc=world["pt_has_desc"])


# ---- worlds ---------------------------------------------------------------------------------------------------------------------------------

def make_world(pw, desc, first_level, K, seed, C=2, max_obs=3, levels=3, eye=(0.0, 0.0, 0.4)):
    """a map on K keyframes around given points: every point has 1 .. max_obs observers (ascending, as the selection wants them) with feature
    indices that are distinct within a keyframe and have gaps; an attribute row per observer in a shuffled order, the first with
    first_level[p]; the centres lie within 2 cm of `eye`, so that every point is usable"""
    rng = np.random.default_rng(seed)
    P = len(pw)
    feats = [list(rng.permutation(2 * P + 8)) for _ in range(K)]
    off, kf, feat, a_off, a_kf, a_level = [0], [], [], [0], [], []
    for p in range(P):
        ks = sorted(rng.choice(K, int(rng.integers(1, min(max_obs, K) + 1)), replace=False).tolist())
        kf += ks
        feat += [int(feats[k].pop()) for k in ks]
        off.append(len(kf))
        rows = list(rng.permutation(ks))
        a_kf += [int(k) for k in rows]
        a_level += [int(first_level[p])] + [int(v) for v in rng.integers(0, levels, len(rows) - 1)]
        a_off.append(len(a_kf))
    cov = np.full((K, C), -1, np.int32)
    for k in range(K):
        others = [c for c in range(K) if c != k]
        n = min(C, len(others))
        cov[k, :n] = rng.choice(others, n, replace=False)
    return dict(K=K, kf_bad=np.zeros(K, np.uint8), C=C, cov=cov, off=np.array(off, np.int32), kf=np.array(kf, np.int32),
                feat=np.array(feat, np.int32), pt_bad=np.zeros(P, np.uint8), center=np.asarray(eye) + rng.uniform(-0.02, 0.02, (K, 3)),
                a_off=np.array(a_off, np.int32), a_kf=np.array(a_kf, np.int32), a_level=np.array(a_level, np.int32),
                pw=np.array(pw, np.float64), pt_desc=np.array(desc, np.uint8), pt_has_desc=np.ones(P, np.uint8))


def copy_world(w):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in w.items()}


def without_rows(w, p):
    """point p loses its attribute rows: state 0"""
    a, b = int(w["a_off"][p]), int(w["a_off"][p + 1])
    w["a_kf"], w["a_level"] = np.delete(w["a_kf"], slice(a, b)), np.delete(w["a_level"], slice(a, b))
    w["a_off"] = w["a_off"].copy()
    w["a_off"][p + 1:] -= b - a
    return w


def on_centre(w, p):
    """point p moves onto the centre of its first row: state 2"""
    w["pw"][p] = w["center"][int(w["a_kf"][int(w["a_off"][p])])]
    return w


def no_desc(w, p):
    w["pt_has_desc"][p] = 0
    return w


def refuse(w, points):
    """the three ways in turn over `points`"""
    for i, p in enumerate(points):
        (without_rows, on_centre, no_desc)[i % 3](w, int(p))
    return w
