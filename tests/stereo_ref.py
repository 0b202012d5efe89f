"""ctypes loader of tests/stereo_ref.c, the restatement of the stereo stage (ygz_slam_amd/csrc/stereo.hip), a numpy witness of the same spec
written another way (vectorised candidate filter and windows, np.sort for the median), and the scenes that tests/test_stereo_ref.py,
tests/test_gpu_stereo.py and tests/test_gpu_stereo_surface.py share.  Test infrastructure: compiled with gcc into a temporary directory the first
time it is used, never imported by the package."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

OK, NO_CANDIDATE, DESCRIPTOR, BORDER, EDGE, DISPARITY, MEDIAN = range(7)
N_STATUS = 7
W, L = 5, 5
# the context's default fx (ygz_hip_default_params: config/default.yaml) as the float it stores, converted to double
DEFAULT_FX = float(np.float32(520.9))
OUTPUTS = ("right_idx", "u_right", "depth", "sad", "status", "counts")
STAGES = ("best_idx", "best_dist", "n_cand", "sads")


class Params(ctypes.Structure):
    """sr_params = ygz_stereo_params"""
    _fields_ = [("baseline", ctypes.c_double), ("min_disparity", ctypes.c_double), ("max_disparity", ctypes.c_double),
                ("th_dist", ctypes.c_int), ("write_depths", ctypes.c_int)]


def params(baseline=0.1, min_disparity=0.0, max_disparity=0.0, th_dist=75, write_depths=1):
    return Params(float(baseline), float(min_disparity), float(max_disparity), int(th_dist), int(write_depths))


def fields(p):
    return {n: getattr(p, n) for n, _ in Params._fields_}


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="stereo_ref_")
        so = os.path.join(d, "libstereo_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "stereo_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        i32, dbl, u8 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
        _lib.sr_match.argtypes = [ctypes.c_int, i32, i32, ctypes.POINTER(u8), ctypes.POINTER(u8), ctypes.c_double,
                                  dbl, i32, u8, ctypes.c_int, dbl, i32, u8, ctypes.c_int, ctypes.POINTER(Params),
                                  i32, dbl, dbl, i32, i32, i32, i32, i32, i32, i32, dbl, i32]
        _lib.sr_match.restype = None
        _lib.sr_median_rule.argtypes = [ctypes.c_int, i32, i32, dbl, dbl, i32]
        _lib.sr_median_rule.restype = None
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def keypoints(px, level, desc):
    """the three arrays of a keypoint list in the ABI's types"""
    return dict(px=np.ascontiguousarray(px, np.float64).reshape(-1, 2), level=np.ascontiguousarray(level, np.int32).reshape(-1),
                desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32))


def head(kp, n):
    return {k: v[:n].copy() for k, v in kp.items()}


def _level_ptrs(levels):
    levels = [np.ascontiguousarray(im, np.uint8) for im in levels]
    arr = (ctypes.POINTER(ctypes.c_uint8) * len(levels))(*[_p(im, ctypes.c_uint8) for im in levels])
    return levels, arr


def match(left, right, kl, kr, p, fx=DEFAULT_FX):
    """sr_match: left, right lists of level images; kl, kr from keypoints().  Every output of the ABI plus the stages, delta and k."""
    left, lp = _level_ptrs(left)
    right, rp = _level_ptrs(right)
    assert [im.shape for im in left] == [im.shape for im in right]
    lw = np.array([im.shape[1] for im in left], np.int32)
    lh = np.array([im.shape[0] for im in left], np.int32)
    nl, nr = len(kl["level"]), len(kr["level"])
    m = max(nl, 1)
    o = dict(right_idx=np.empty(m, np.int32), u_right=np.empty(m), depth=np.empty(m), sad=np.empty(m, np.int32), status=np.empty(m, np.int32),
             counts=np.empty(N_STATUS, np.int32), best_idx=np.empty(m, np.int32), best_dist=np.empty(m, np.int32), n_cand=np.empty(m, np.int32),
             sads=np.empty((m, 2 * L + 1), np.int32), delta=np.empty(m), k=np.empty(m, np.int32))
    i32, dbl, u8 = ctypes.c_int32, ctypes.c_double, ctypes.c_uint8
    pad = lambda a: a if len(a) else np.zeros((1,) + a.shape[1:], a.dtype)
    a, b = {k: pad(v) for k, v in kl.items()}, {k: pad(v) for k, v in kr.items()}
    lib().sr_match(len(left), _p(lw, i32), _p(lh, i32), lp, rp, float(fx), _p(a["px"], dbl), _p(a["level"], i32), _p(a["desc"], u8), nl,
                   _p(b["px"], dbl), _p(b["level"], i32), _p(b["desc"], u8), nr, ctypes.byref(p),
                   _p(o["right_idx"], i32), _p(o["u_right"], dbl), _p(o["depth"], dbl), _p(o["sad"], i32), _p(o["status"], i32), _p(o["counts"], i32),
                   _p(o["best_idx"], i32), _p(o["best_dist"], i32), _p(o["n_cand"], i32), _p(o["sads"], i32), _p(o["delta"], dbl), _p(o["k"], i32))
    return {k: (v if k == "counts" else v[:nl]) for k, v in o.items()}


def median_rule(status, sad):
    """sr_median_rule on hand-made lists: (status, counts)"""
    st, sd = np.ascontiguousarray(status, np.int32).copy(), np.ascontiguousarray(sad, np.int32)
    counts = np.empty(N_STATUS, np.int32)
    n = len(st)
    if n == 0:
        st, sd = np.zeros(1, np.int32), np.zeros(1, np.int32)
    lib().sr_median_rule(n, _p(st, ctypes.c_int32), _p(sd, ctypes.c_int32), None, None, _p(counts, ctypes.c_int32))
    return st[:n], counts


def witness_median(status, sad):
    st = np.array(status, np.int64).copy()
    sd = np.array(sad, np.int64)
    ok = st == OK
    if ok.any():
        med = np.sort(sd[ok])[int(ok.sum()) // 2]
        st[ok & (10 * sd > 21 * med)] = MEDIAN
    return st.astype(np.int32), np.bincount(st, minlength=N_STATUS).astype(np.int32)


def witness(left, right, kl, kr, p, fx=DEFAULT_FX):
    """the spec again, in numpy: one vectorised candidate filter per left keypoint, the SAD of all eleven columns from one sliding-window view"""
    from numpy.lib.stride_tricks import sliding_window_view
    nl = len(kl["level"])
    bf, mind, maxd = fx * p.baseline, p.min_disparity, (p.max_disparity if p.max_disparity != 0.0 else fx)
    o = dict(right_idx=np.full(nl, -1, np.int32), u_right=np.full(nl, -1.0), depth=np.full(nl, -1.0), sad=np.full(nl, -1, np.int32),
             status=np.full(nl, NO_CANDIDATE, np.int32), best_idx=np.full(nl, -1, np.int32), best_dist=np.full(nl, -1, np.int32),
             n_cand=np.zeros(nl, np.int32), sads=np.full((nl, 2 * L + 1), -1, np.int32), delta=np.zeros(nl), k=np.full(nl, -99, np.int32))
    ur, vr, lr = kr["px"][:, 0], kr["px"][:, 1], kr["level"].astype(np.int64)
    band = 2.0 * np.exp2(lr)
    top, bottom = np.floor(vr - band), np.ceil(vr + band)
    bits_l, bits_r = np.unpackbits(kl["desc"], axis=1), np.unpackbits(kr["desc"], axis=1)
    for i in range(nl):
        ul, vl, l = float(kl["px"][i, 0]), float(kl["px"][i, 1]), int(kl["level"][i])
        if ul - mind < 0:
            continue
        cand = np.nonzero((np.abs(lr - l) <= 1) & (top <= np.floor(vl)) & (np.floor(vl) <= bottom) & (ur >= ul - maxd) & (ur <= ul - mind))[0]
        o["n_cand"][i] = len(cand)
        if not len(cand):
            continue
        dist = (bits_r[cand] != bits_l[i]).sum(axis=1)
        b = int(np.argmin(dist))
        j = int(cand[b])
        o["best_idx"][i], o["best_dist"][i] = j, dist[b]
        if dist[b] >= p.th_dist:
            o["status"][i] = DESCRIPTOR
            continue
        s = float(2 ** l)
        su, sv, sr = int(np.floor(ul / s + 0.5)), int(np.floor(vl / s + 0.5)), int(np.floor(float(ur[j]) / s + 0.5))
        il, ir = left[l].astype(np.int64), right[l].astype(np.int64)
        hl, wl = il.shape
        if not (W <= su < wl - W and W <= sv < hl - W and sr - L - W >= 0 and sr + L + W < wl):
            o["status"][i] = BORDER
            continue
        a = il[sv - W:sv + W + 1, su - W:su + W + 1] - il[sv, su]
        wins = sliding_window_view(ir[sv - W:sv + W + 1, sr - L - W:sr + L + W + 1], (2 * W + 1, 2 * W + 1))[0]      # [11 columns][11][11]
        d = np.abs(a[None] - (wins - ir[sv, sr - L:sr + L + 1][:, None, None])).sum(axis=(1, 2))
        o["sads"][i] = d
        q = int(np.argmin(d))
        o["k"][i] = q - L
        if q == 0 or q == 2 * L:
            o["status"][i] = EDGE
            continue
        d1, d2, d3 = int(d[q - 1]), int(d[q]), int(d[q + 1])
        delta = float(d1 - d3) / float(2 * (d1 + d3 - 2 * d2))
        o["delta"][i] = delta
        urs = s * (float(sr + q - L) + delta)
        disp = ul - urs
        if not (mind <= disp < maxd):
            o["status"][i] = DISPARITY
            continue
        if disp <= 0:
            disp, urs = 0.01, ul - 0.01
        o["status"][i], o["right_idx"][i], o["u_right"][i], o["depth"][i], o["sad"][i] = OK, j, urs, bf / disp, d2
    st, counts = witness_median(o["status"], o["sad"])
    lost = (o["status"] == OK) & (st == MEDIAN)
    o["u_right"][lost] = -1.0
    o["depth"][lost] = -1.0
    o["status"], o["counts"] = st, counts
    return o


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------

def _box(t, n):
    return sum(t[dy:t.shape[0] - n + 1 + dy, dx:t.shape[1] - n + 1 + dx] for dy in range(n) for dx in range(n)) / float(n * n)


def texture(w, h, seed, cell=4, fine=0.5):
    """uniform noise at two scales in the parts (fine, 1 - fine): one sample per pixel box-filtered twice (3 x 3), and one per cell x cell pixels
    box-filtered twice (cell x cell), so that the 11 x 11 window sees structure of its own scale at level 0 and at level 2, and no two patches
    are alike"""
    rng = np.random.default_rng(seed)
    f = _box(_box(rng.integers(0, 256, (h + 4, w + 4)).astype(np.float64), 3), 3)
    hc, wc = (h + cell - 1) // cell + 2, (w + cell - 1) // cell + 2
    c = _box(_box(np.kron(rng.integers(0, 256, (hc, wc)).astype(np.float64), np.ones((cell, cell))), cell), cell)[:h, :w]
    t = fine * (f - f.mean()) * 4.0 + (1.0 - fine) * (c - c.mean()) + 128.0            # the filters shrink the contrast: stretch it back
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def shifted_pair(w, h, shift, seed, **kw):
    """right(x) = left(x + shift), the uncovered columns from the same texture source"""
    src = texture(w + shift, h, seed, **kw)
    return np.ascontiguousarray(src[:, :w]), np.ascontiguousarray(src[:, shift:shift + w])


def lattice(w, h, step=12):
    """hand-placed keypoints on a lattice, levels cycling 0, 1, 2: (px [n, 2], level [n])"""
    pts = [(x, y) for y in range(step, h, step) for x in range(step, w, step)]
    return np.array(pts, np.float64), (np.arange(len(pts)) % 3).astype(np.int32)


def described(oracle, levels, px, level):
    from oracle.pyoracle import KP_DTYPE
    k = np.zeros(len(level), KP_DTYPE)
    k["px"], k["py"], k["level"] = px[:, 0], px[:, 1], level
    k = oracle.describe(levels, k)
    return keypoints(px, level, k["desc"])


class Scene(object):
    """left / right: lists of level images; kl / kr: keypoint lists; twin [nl]: the right index of each left keypoint's twin (-1: none);
    shift: the disparity of the pictures"""

    def __init__(self, left, right, kl, kr, twin, shift):
        self.left, self.right, self.kl, self.kr, self.twin, self.shift = left, right, kl, kr, np.asarray(twin, np.int32), shift


_scenes = {}


def scene(oracle, name):
    """the scenes of tests/test_stereo_ref.py by name: 'a' three-level shift 8, 'b' = a + noise on the right half of the right picture,
    'c' identical pictures, 'd' the mirror picture (34 x 32, level 0), 'e' shift 32 with offset twins"""
    if name not in _scenes:
        _scenes[name] = {"a": _scene_a, "b": _scene_b, "c": _scene_c, "d": _scene_d, "e": _scene_e}[name](oracle)
    return _scenes[name]


def _twins(oracle, w, h, shift, seed, noise=False):
    left, right = shifted_pair(w, h, shift, seed)
    if noise:
        rng = np.random.default_rng(seed + 1)
        r = right.astype(np.int64)
        r[:, w // 2:] += rng.integers(-6, 7, (h, w - w // 2))
        right = np.clip(r, 0, 255).astype(np.uint8)
    pl, pr = oracle.pyramid(left, 3), oracle.pyramid(right, 3)
    px, lv = lattice(w, h)
    keep = px[:, 0] - shift >= 0
    kl = described(oracle, pl, px, lv)
    kr = described(oracle, pr, px[keep] - np.array([float(shift), 0.0]), lv[keep])
    twin = np.full(len(lv), -1, np.int32)
    twin[keep] = np.arange(int(keep.sum()))
    return Scene(pl, pr, kl, kr, twin, shift)


def _scene_a(oracle):
    return _twins(oracle, 320, 240, 8, 11)


def _scene_b(oracle):
    return _twins(oracle, 320, 240, 8, 11, noise=True)


def _scene_c(oracle):
    return _twins(oracle, 320, 240, 0, 12)


def _scene_d(oracle):
    """34 x 32, level 0 only: the picture mirrored about column 16; keypoints at every column of row 16 in both lists (the one on column 16 has
    d1 = d3 and disparity 0: the 0.01 branch) """
    w, h, c = 34, 32, 16
    img = texture(w, h, 13)
    img[:, c + 1:2 * c + 1] = img[:, c - 1::-1][:, :c]
    assert np.array_equal(img[:, c - 10:c], img[:, c + 10:c:-1])
    lv = [np.ascontiguousarray(img)]
    px = np.array([(x, 16) for x in range(w)], np.float64)
    k = described(oracle, lv, px, np.zeros(w, np.int32))
    return Scene(lv, lv, k, head(k, w), np.arange(w), 0)


def _scene_e(oracle):
    """shift 32; the right keypoints carry the left descriptors: even left keypoints have their twin 6 * 2^l to the right of where it belongs
    (the true column is outside the search: EDGE), odd ones 4 * 2^l (OK with k = -4); the first eight right keypoints are repeated at the
    end of the list (a tie in the descriptor distance goes to the lower index)"""
    w, h, shift = 320, 240, 32
    left, right = shifted_pair(w, h, shift, 16, cell=16, fine=0.0)          # smooth at every level, so the SAD falls towards the true column (a seed that puts no window of the offset set on a flat spot)
    pl, pr = oracle.pyramid(left, 3), oracle.pyramid(right, 3)
    px, lv = lattice(w, h)
    kl = described(oracle, pl, px, lv)
    keep = np.nonzero(px[:, 0] - shift >= 0)[0]
    off = np.where(keep % 2 == 0, 6.0, 4.0) * np.exp2(lv[keep])
    pr_px = px[keep] + np.stack([off - shift, np.zeros(len(keep))], axis=1)
    twin = np.full(len(lv), -1, np.int32)
    twin[keep] = np.arange(len(keep))
    kr = keypoints(np.concatenate([pr_px, pr_px[:8]]), np.concatenate([lv[keep], lv[keep][:8]]), np.concatenate([kl["desc"][keep], kl["desc"][keep][:8]]))
    return Scene(pl, pr, kl, kr, twin, shift)


def detector_pair(oracle, w, h, shift, seed, other_seed=None):
    """a pair of pictures with shift `shift` (other_seed: an unrelated right picture), as [h, w] uint8"""
    if other_seed is not None:
        return texture(w, h, seed), texture(w, h, other_seed)
    return shifted_pair(w, h, shift, seed)
