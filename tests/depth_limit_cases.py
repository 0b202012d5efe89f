"""Crafted cases that put one input ON each limit of stereo map-point creation (ygz_slam_amd/csrc/smap.hip: k_smap_pairs; DESIGN.md section
24 (a)) and of the stereo depths (csrc/stereo.hip: k_stereo_match, k_stereo_median; section 19).  tests/test_depth_limit_cases.py holds them
to the restatements (tests/smap_ref.c, tests/stereo_ref.c) and to a numpy witness on the CPU, tests/test_gpu_depth_limits.py runs them on the
device.  The literals are written from the numbered steps of the two sections, not from any implementation's output.

Everything is built so that the compared quantities are exact in FP64 and "on the limit" means equality.  Pairs: intrinsics KP = (512, 512,
320, 240), identity poses or the exact quaternions (0,0,0,1), (1/2,1/2,1/2,1/2), (1,0,0,0), dyadic depths, pixels and translations, baseline
0.125 (bf = 64).  Depths: a 320 x 240 context of three levels with fx = 256, baseline 0.125 (bf = 32), keypoints on dyadic coordinates, an
all-zero left picture and right pictures that are zero (every window sum is 0: a keypoint that reaches the SAD search is EDGE, one that
fails the border test is BORDER with sads -1) or zero with single marked pixels (the eleven sums are designed, see STRIPS and BLOBS).  One step
beyond a limit is np.nextafter on a STORED input (a pixel, a depth, a parameter), and the module asserts where it builds the case that the
step changes the compared quantity.  No random number is drawn anywhere.

A pair case is Pair(name, row, K4, pb, params, expected): pb one problem of one pair in the form of smap_ref, expected (code, method,
pos_world or None); pos_world is compared bit for bit.  A depth case is Depth(name, row, right, kl, kr, params, expected): right the name
of the right picture, expected field -> list over the left keypoints (counts: the seven counts)."""
import collections

import numpy as np

# ---- shared ------------------------------------------------------------------------------------------------------------------------------------


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def bits(d):
    """a descriptor with the first d bits set: Hamming distance d from the zero descriptor"""
    return np.packbits(np.arange(256) < d)


def equal_bits(got, want):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(np.asarray(want, got.dtype).reshape(got.shape))
    return got.tobytes() == want.tobytes()


# ==== map-point pairs (section 24 (a)) ==========================================================================================================
KP = (512.0, 512.0, 320.0, 240.0)
KE = (420.0, 421.5, 318.25, 243.125)                    # the camera of smap_ref's scenes, for its two hand-made pairs
ID = (0.0, 0.0, 0.0, 1.0)
PERM = (0.5, 0.5, 0.5, 0.5)                             # R = [[0,0,1],[1,0,0],[0,1,0]]
FLIP = (1.0, 0.0, 0.0, 0.0)                             # R = diag(1, -1, -1)
OPEN = 2.0 ** 40                                        # a chi-square limit no finite error of a case reaches
PAIR_PARAMS = dict(baseline=0.125, chi2_mono=4.0, chi2_stereo=8.0, cos_parallax_max=0.9998, ratio_factor=16.0)
NAN = float("nan")
PAIR_POSITIONS = (0, 63, 64, 256)
N_EMBED = 257
PROBLEM_POSITIONS = (0, 15, 31)
N_PROBLEMS = 32
# cameras of the neighbours in the 32-problem form: rotations about y by 2 atan(3/4) and by 2 atan(7/24), translations of metres.  Under them
# every case ends otherwise than its literal says (tests/test_depth_limit_cases.py checks it), so reading a neighbour's cameras shows
NEIGHBOUR_T1 = (0.0, 0.6, 0.0, 0.8, 1.0, -2.0, 3.0)
NEIGHBOUR_T2 = (0.0, 0.28, 0.0, 0.96, -3.0, 1.0, 2.0)
OK, NO_METHOD, DEGENERATE, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, SCALE = range(9)

Pair = collections.namedtuple("Pair", "name row K4 pb params expected")


def pose(q=ID, t=(0.0, 0.0, 0.0)):
    return tuple(float(a) for a in q) + tuple(float(a) for a in t)


def cos_stereo(d, b):
    """step 2's closed form in the restatement's order of operations"""
    h = 0.5 * b
    return (d * d - h * h) / (d * d + h * h)


def cos_rays(xn1, xn2):
    """step 1 for two cameras of identity rotation"""
    dot = (xn1[0] * xn2[0] + xn1[1] * xn2[1]) + 1.0
    n1 = float(np.sqrt((xn1[0] * xn1[0] + xn1[1] * xn1[1]) + 1.0))
    n2 = float(np.sqrt((xn2[0] * xn2[0] + xn2[1] * xn2[1]) + 1.0))
    return dot / (n1 * n2)


def pair(row, name, code, method, pos=None, T1=pose(), T2=pose(), px1=(320.0, 240.0), px2=(320.0, 240.0), ur1=-1.0, ur2=-1.0, d1=NAN, d2=NAN,
         l1=0, l2=0, K4=KP, **params):
    """one pair.  A mono side's depth is NaN unless the case puts a value there that must not be read"""
    assert not (ur1 >= 0 and np.isnan(d1)) and not (ur2 >= 0 and np.isnan(d2))          # the entry point refuses a stereo side without a depth
    pb = dict(T1=np.array(T1, np.float64), T2=np.array(T2, np.float64), px1=np.array([px1], np.float64), px2=np.array([px2], np.float64),
              ur1=np.array([ur1], np.float64), ur2=np.array([ur2], np.float64), depth1=np.array([d1], np.float64),
              depth2=np.array([d2], np.float64), level1=np.array([l1], np.int32), level2=np.array([l2], np.int32), n=1)
    prm = dict(PAIR_PARAMS, **params) if K4 is KP else dict(params)
    return Pair("pair/%s/%s" % (row, name), row, K4, pb, prm, (code, method, None if pos is None else tuple(float(a) for a in pos)))


def _ur_cases():
    """row 1.  Pixel (16, 240) at depth 4 has the right column 16 - 64 / 4 = 0: ur = 0.0 is a consistent stereo measurement.  Both cameras
    are the identity, so the rays are parallel and a stereo side un-projects; without one the pair is mono-mono with cosRays above 0.9998"""
    r, p, X = "ur", (16.0, 240.0), (-2.375, 0.0, 4.0)
    return [pair(r, "ur1=+0", OK, 2, X, px1=p, px2=p, ur1=0.0, d1=4.0),
            pair(r, "ur1=-0", OK, 2, X, px1=p, px2=p, ur1=-0.0, d1=4.0),
            pair(r, "ur1 below 0, its depth not read", NO_METHOD, 0, px1=p, px2=p, ur1=down(0.0), d1=4.0),
            pair(r, "ur2=+0", OK, 3, X, px1=p, px2=p, ur2=0.0, d2=4.0),
            pair(r, "ur2=-0", OK, 3, X, px1=p, px2=p, ur2=-0.0, d2=4.0),
            pair(r, "ur2 below 0, its depth not read", NO_METHOD, 0, px1=p, px2=p, ur2=down(0.0), d2=4.0)]


def _cos_stereo_cases():
    """row 2.  Rays (0,0,1) and (3/4,0,1): cosRays = 1 / 1.25 = 0.8; b = 0.125, d = 0.1875: cosS = 0.03125 / 0.0390625 = 0.8.  Camera 2 is
    0.140625 to the left, so the un-projected point (0, 0, 0.1875) lands on pixel 704 of camera 2; the gates are open"""
    r, kw = "cosRays==cosS", dict(px2=(704.0, 240.0), T2=pose(t=(0.140625, 0.0, 0.0)), ur1=0.0, chi2_mono=OPEN, chi2_stereo=OPEN)
    on, step = 0.8, cos_rays((0.0, 0.0), ((up(704.0) - 320.0) / 512.0, 0.0))
    assert cos_rays((0.0, 0.0), (0.75, 0.0)) == on == cos_stereo(0.1875, 0.125) and step < on
    return [pair(r, "on", OK, 2, (0.0, 0.0, 0.1875), d1=0.1875, **kw),
            pair(r, "cosRays one step below", OK, 1, d1=0.1875, **dict(kw, px2=(up(704.0), 240.0)))]


def _cos_zero_cases():
    """row 3.  Camera 2 turned by the axis permutation: its optical axis is the world's y axis, ray2 = (xn2.y, 1, xn2.x), so
    cosRays = xn2.x / |ray2| and the principal point gives exactly 0.  It sits where the point (0,0,4) is 4 in front of it"""
    r, kw = "cosRays==0", dict(T2=pose(PERM, (-4.0, 0.0, 4.0)), ur1=304.0, d1=4.0)
    assert (up(320.0) - 320.0) / 512.0 > 0.0 > (down(320.0) - 320.0) / 512.0
    return [pair(r, "on", OK, 2, (0.0, 0.0, 4.0), **kw),
            pair(r, "one step above", OK, 1, px2=(up(320.0), 240.0), **kw),
            pair(r, "one step below", OK, 2, (0.0, 0.0, 4.0), px2=(down(320.0), 240.0), **kw)]


def _parallax_cases():
    """row 4.  The rays of row 2 between two mono sides: cosRays = 0.8 against cos_parallax_max = 0.8.  Camera 2 is 3 to the left: the
    rays meet at (0,0,4)"""
    r, kw = "cos_parallax_max", dict(px2=(704.0, 240.0), T2=pose(t=(3.0, 0.0, 0.0)), chi2_mono=OPEN, chi2_stereo=OPEN)
    assert up(0.8) > 0.8
    return [pair(r, "on", NO_METHOD, 0, cos_parallax_max=0.8, **kw),
            pair(r, "limit one step above", OK, 1, cos_parallax_max=up(0.8), **kw),
            pair(r, "a stereo side ignores the gate", OK, 1, ur1=304.0, d1=4.0, cos_parallax_max=0.8, **kw)]


def _asymmetry_cases():
    """row 5.  (a) both sides stereo: depth2 = 0.1875 would make cosS2 = 0.8 = cosRays and forbid the triangulation.  (b, c) parallel
    rays: side 2 un-projects only when side 1 is mono.  (d) the tie cosS1 == cosS2 exists for antiparallel rays (cosS2 = cosRays + 1 = 0)
    and depth1 = b / 2 (cosS1 = 0); camera 2 looks back from (0,0,1)"""
    r, gates = "asymmetry", dict(chi2_mono=OPEN, chi2_stereo=OPEN)
    out = [pair(r, "side 2's depth not used", OK, 1, px2=(704.0, 240.0), T2=pose(t=(3.0, 0.0, 0.0)), ur1=304.0, d1=4.0, ur2=0.0, d2=0.1875, **gates),
           pair(r, "method 3: side 1 mono", OK, 3, (0.0, 0.0, 4.0), ur2=304.0, d2=4.0, **gates),
           pair(r, "method 2: side 1 stereo too", OK, 2, (0.0, 0.0, 8.0), ur1=312.0, d1=8.0, ur2=304.0, d2=4.0, **gates)]
    h, back = 0.0625, pose(FLIP, (0.0, 0.0, 1.0))
    assert cos_stereo(h, 0.125) == 0.0 and cos_stereo(down(h), 0.125) < 0.0 < cos_stereo(up(h), 0.125)
    out += [pair(r, "tie, side 1", NO_METHOD, 0, T2=back, ur1=0.0, d1=h, **gates),
            pair(r, "tie, side 1, depth one step below", OK, 2, (0.0, 0.0, down(h)), T2=back, ur1=0.0, d1=down(h), **gates),
            pair(r, "tie, side 1, depth one step above", NO_METHOD, 0, T2=back, ur1=0.0, d1=up(h), **gates),
            pair(r, "tie, side 2", NO_METHOD, 0, T2=back, ur2=0.0, d2=h, **gates),
            pair(r, "tie, side 2, depth one step below", OK, 3, (0.0, 0.0, 1.0 - down(h)), T2=back, ur2=0.0, d2=down(h), **gates),
            pair(r, "tie, side 2, depth one step above", NO_METHOD, 0, T2=back, ur2=0.0, d2=up(h), **gates)]
    return out


def _behind_cases():
    """row 6.  Un-projection from camera 1 (the identity) puts the point at z1 = depth1; camera 2 sees it at z2 = depth1 + t2.z.  The
    smallest positive z1 goes on and fails the stereo reprojection (bf / z is infinite); the smallest positive z2 goes on to the scale
    test, where dist2 / dist1 is 1e-16"""
    r = "z>0"
    assert 4.0 + up(-4.0) > 0.0 and 4.0 + -4.0 == 0.0
    return [pair(r, "z1=0", BEHIND_1, 2, ur1=0.0, d1=0.0, T2=pose(t=(0.0, 0.0, 1.0))),
            pair(r, "z1 one step above 0", REPROJ_1, 2, ur1=0.0, d1=5e-324, T2=pose(t=(0.0, 0.0, 1.0))),
            pair(r, "z2=0", BEHIND_2, 2, ur1=304.0, d1=4.0, T2=pose(t=(0.0, 0.0, -4.0))),
            pair(r, "z2 one step above 0", SCALE, 2, ur1=304.0, d1=4.0, T2=pose(t=(0.0, 0.0, up(-4.0)))),
            pair(r, "both fail", BEHIND_1, 2, ur1=0.0, d1=0.0)]


def _reprojection_cases():
    """row 7.  The point (0,0,4) un-projected from the stereo side (pixel (320,240), ur 304, depth 4) is seen by the other camera, 1/32 to
    the left, at u = 324, ur = 308.  The other side's pixel is `off` away: mono e2 = off^2 against 4 * 4^level, stereo e2 = 2 off^2 against
    8 * 4^level.  Then the stereo side's own column error against chi2_stereo = 16.  Mirrored (camera 1 moved, side 2 stereo) for code 5
    of a mono side"""
    r, out = "reprojection", []
    moved, X = pose(t=(0.03125, 0.0, 0.0)), (0.0, 0.0, 4.0)
    one = dict(T2=moved, ur1=304.0, d1=4.0)
    two = dict(T1=moved, ur2=304.0, d2=4.0)
    for l in (0, 1, 2):
        off = 2.0 * 2 ** l
        x = 324.0 - off
        assert (324.0 - down(x)) ** 2 > off * off == 4.0 * 4 ** l and (308.0 - down(308.0 - off)) ** 2 + off * off > 2 * off * off == 8.0 * 4 ** l
        out += [pair(r, "mono side 2, level %d, on" % l, OK, 2, X, px2=(x, 240.0), l2=l, **one),
                pair(r, "mono side 2, level %d, one step" % l, REPROJ_2, 2, px2=(down(x), 240.0), l2=l, **one),
                pair(r, "stereo side 2, level %d, on" % l, OK, 2, X, px2=(x, 240.0), ur2=308.0 - off, d2=4.0, l2=l, **one),
                pair(r, "stereo side 2, level %d, one step" % l, REPROJ_2, 2, px2=(x, 240.0), ur2=down(308.0 - off), d2=4.0, l2=l, **one),
                pair(r, "mono side 1, level %d, on" % l, OK, 3, X, px1=(x, 240.0), l1=l, **two),
                pair(r, "mono side 1, level %d, one step" % l, REPROJ_1, 3, px1=(down(x), 240.0), l1=l, **two)]
        er = 4.0 * 2 ** l
        assert (304.0 - down(304.0 - er)) ** 2 > er * er == 16.0 * 4 ** l
        out += [pair(r, "stereo side 1, level %d, on" % l, OK, 2, X, T2=moved, px2=(324.0, 240.0), ur1=304.0 - er, d1=4.0, l1=l, chi2_stereo=16.0),
                pair(r, "stereo side 1, level %d, one step" % l, REPROJ_1, 2, T2=moved, px2=(324.0, 240.0), ur1=down(304.0 - er), d1=4.0, l1=l,
                     chi2_stereo=16.0)]
    out += [  # the level is the side's own: e2 = 16 passes at level 1 and fails at level 0, whatever the other side's level is
        pair(r, "side 2 at level 1, side 1 at level 0", OK, 2, X, px2=(320.0, 240.0), l1=0, l2=1, **one),
        pair(r, "side 2 at level 0, side 1 at level 1", REPROJ_2, 2, px2=(320.0, 240.0), l1=1, l2=0, **one),
        pair(r, "side 1 at level 1, side 2 at level 0", OK, 3, X, px1=(320.0, 240.0), l1=1, l2=0, **two),
        pair(r, "side 1 at level 0, side 2 at level 1", REPROJ_1, 3, px1=(320.0, 240.0), l1=0, l2=1, **two),
        # code 5 comes before code 6: side 1's column is 4 off (16 > 8) and side 2's pixel 14 off
        pair(r, "both sides fail", REPROJ_1, 2, T2=moved, px2=(310.0, 240.0), ur1=300.0, d1=4.0),
        pair(r, "side 2 alone fails", REPROJ_2, 2, T2=moved, px2=(310.0, 240.0), ur1=304.0, d1=4.0),
        # ur2 = 0.0 is a stereo measurement: the column error is 308
        pair(r, "ur2=0.0 takes the stereo formula", REPROJ_2, 2, px2=(324.0, 240.0), ur2=0.0, d2=4.0, **one),
        pair(r, "ur2 below 0 takes the mono formula", OK, 2, X, px2=(324.0, 240.0), ur2=down(0.0), **one)]
    return out


def _scale_cases():
    """row 8.  Both cameras on the optical axis of camera 1, the point at (0,0,4): dist1 = 4, dist2 = 4 + t2.z = 2 or 8, ratio_factor 2"""
    r, out, X = "scale", [], (0.0, 0.0, 4.0)
    assert 0.5 * down(2.0) < 1.0 and 2.0 > 1.0 * down(2.0) and 2.0 * down(2.0) < 4.0 and 0.5 > 0.25 * down(2.0)
    for name, l1, l2, tz in (("lower, levels (1,1)", 1, 1, -2.0), ("upper, levels (1,1)", 1, 1, 4.0), ("lower, levels (2,0)", 2, 0, 4.0),
                             ("upper, levels (0,2)", 0, 2, -2.0)):
        kw = dict(T2=pose(t=(0.0, 0.0, tz)), ur1=304.0, d1=4.0, l1=l1, l2=l2)
        out += [pair(r, name + ", on", OK, 2, X, ratio_factor=2.0, **kw), pair(r, name + ", one step", SCALE, 2, ratio_factor=down(2.0), **kw)]
    return out


def _hand_made_cases():
    """row 9: the two pairs of smap_ref.edge_cases(), written out (its camera, the library's default parameters)"""
    fx, fy, cx, cy = KE
    dflt = dict(baseline=0.1, chi2_mono=5.991, chi2_stereo=7.8, cos_parallax_max=0.9998, ratio_factor=3.0)
    return [pair("hand-made", "code 2", DEGENERATE, 1, T2=pose(t=(-1.0, 0.0, 0.0)), px1=(cx, cy), px2=(cx, cy), d1=0.0, d2=0.0, K4=KE,
                 **dict(dflt, cos_parallax_max=2.0)),
            pair("hand-made", "code 7", ZERO_DIST, 2, T2=pose(PERM, (-1.0, 0.0, 0.0)), px1=(cx, fy * 1e-170), px2=(cx - 1.0, 0.0), ur1=cx - fx * 0.1,
                 d1=1.0, d2=0.0, K4=(fx, fy, cx, 0.0), **dflt)]


PAIR_ROWS = ("ur", "cosRays==cosS", "cosRays==0", "cos_parallax_max", "asymmetry", "z>0", "reprojection", "scale", "hand-made")
_pairs = None


def pair_cases():
    global _pairs
    if _pairs is None:
        out = (_ur_cases() + _cos_stereo_cases() + _cos_zero_cases() + _parallax_cases() + _asymmetry_cases() + _behind_cases() +
               _reprojection_cases() + _scale_cases() + _hand_made_cases())
        assert len({c.name for c in out}) == len(out)
        _pairs = out
    return list(_pairs)


def filler(case):
    """(the pair that fills the other 256 places of the embedded form, its code).  A stereo side 1 at depth 0 at the principal point
    un-projects to camera 1's centre, z1 = 0: code 3 whatever camera 2 is (cosS1 = -1 is below every cosRays + 1).  For the cases that are
    code 3 themselves, two mono sides at the principal point of cameras of one rotation: parallel rays, code 1"""
    c = (case.K4[2], case.K4[3])
    if case.expected[0] == BEHIND_1:
        return dict(px1=c, px2=c, ur1=-1.0, ur2=-1.0, depth1=NAN, depth2=NAN, level1=0, level2=0), NO_METHOD
    return dict(px1=c, px2=c, ur1=0.0, ur2=-1.0, depth1=0.0, depth2=NAN, level1=0, level2=0), BEHIND_1


def pair_at(case, pos):
    """the problem of N_EMBED pairs with the case's pair at index pos and filler(case) everywhere else"""
    f, _ = filler(case)
    pb = dict(T1=case.pb["T1"], T2=case.pb["T2"], n=N_EMBED)
    for k, v in f.items():
        a = np.asarray(case.pb[k])
        full = np.empty((N_EMBED,) + a.shape[1:], a.dtype)
        full[:] = v
        full[pos] = a[0]
        pb[k] = full
    return pb


def problems_around(case, pos):
    """N_PROBLEMS problems with the case as problem pos: the problems next to it and every fourth one are empty, the others hold the
    case's pair under the neighbours' cameras"""
    empty = dict(T1=np.array(NEIGHBOUR_T2), T2=np.array(NEIGHBOUR_T1), n=0)
    for k, v in case.pb.items():
        if k not in ("T1", "T2", "n"):
            empty[k] = v[:0]
    other = dict(case.pb, T1=np.array(NEIGHBOUR_T1), T2=np.array(NEIGHBOUR_T2))
    return [case.pb if q == pos else (empty if abs(q - pos) == 1 or q % 4 == 3 else other) for q in range(N_PROBLEMS)]


def pair_families(cases):
    """the cases that may share a call: one K4, one parameter set"""
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault((c.K4, tuple(sorted(c.params.items()))), []).append(c)
    return list(out.values())


def pair_holds(case, code, method, pos):
    """what of the case's literal (code, method, pos_world) the outputs of its pair miss"""
    want_code, want_method, want_pos = case.expected
    bad = [n for n, a, b in (("code", int(code), want_code), ("method", int(method), want_method)) if a != b]
    if want_code != OK and not equal_bits(np.asarray(pos, np.float64), (0.0, 0.0, 0.0)):
        bad.append("pos_world")
    if want_pos is not None and not equal_bits(np.asarray(pos, np.float64), want_pos):
        bad.append("pos_world")
    return bad


# ==== stereo depths (section 19) ================================================================================================================
WIDTH, HEIGHT, LEVELS = 320, 240, 3
FX = 256.0
INTRINSICS = (256.0, 256.0, 160.0, 120.0)
BF = 32.0                                               # fx * baseline
DEPTH_PARAMS = dict(baseline=0.125, min_disparity=0.0, max_disparity=0.0, th_dist=75, write_depths=0)
S_OK, NO_CANDIDATE, DESCRIPTOR, BORDER, EDGE, DISPARITY, MEDIAN = range(7)
NONE11, ZERO11 = [-1] * 11, [0] * 11

Depth = collections.namedtuple("Depth", "name row right kl kr params expected")


def kps(entries):
    """a keypoint list from (u, v, level, descriptor or its distance from zero)"""
    desc = [bits(e[3]) if np.isscalar(e[3]) else np.asarray(e[3], np.uint8) for e in entries]
    return dict(px=np.array([(e[0], e[1]) for e in entries], np.float64).reshape(-1, 2), level=np.array([e[2] for e in entries], np.int32),
                desc=np.array(desc, np.uint8).reshape(-1, 32))


def depth(row, name, left, right_kps, expected, right="zero", **params):
    return Depth("depth/%s/%s" % (row, name), row, right, kps(left), kps(right_kps), dict(DEPTH_PARAMS, **params), expected)


def flat(status, n_cand=1):
    """what ONE left keypoint over the zero pictures ends as: EDGE when it reaches the SAD search (all eleven sums are 0, the first is the
    smallest), BORDER or an earlier status otherwise"""
    return dict(status=[status], n_cand=[n_cand], sads=[ZERO11 if status == EDGE else NONE11], right_idx=[-1], sad=[-1], u_right=[-1.0], depth=[-1.0])


def _step1_cases():
    r = "uL-minD"
    assert 8.0 - 8.0 == 0.0 and down(8.0) - 8.0 < 0.0
    return [depth(r, "on", [(8.0, 100.0, 0, 0)], [(0.0, 100.0, 0, 0)], dict(flat(BORDER), best_idx=[0]), min_disparity=8.0),
            depth(r, "one step below", [(down(8.0), 100.0, 0, 0)], [(-1.0, 100.0, 0, 0)], dict(flat(NO_CANDIDATE, 0), best_idx=[-1]), min_disparity=8.0)]


def _level_cases():
    r, out = "level gate", []
    for l in range(LEVELS):
        for lr in range(LEVELS):
            ok = abs(lr - l) <= 1
            out.append(depth(r, "l=%d lr=%d" % (l, lr), [(200.0, 100.0, l, 0)], [(180.0, 100.0, lr, 0)],
                             dict(flat(EDGE if ok else NO_CANDIDATE, int(ok)), best_idx=[0 if ok else -1])))
    return out


def _band_cases():
    """row 3.  r = 2 * 2^lr of the RIGHT level.  Below the left keypoint: vL just above 100 (floor 100), vR = 101 + r is refused
    (floor(vR - r) = 101) and the double below it admitted; this is also the farthest row above vL that the band admits, 1 + r away.
    Above it: vL just below 101 (floor 100), vR = 99 - r is refused (ceil(vR + r) = 99) and the double above it admitted, 2 + r away: for
    lr = l + 1 that is 2 + 4 * 2^l, inside the kernel's early cull of 4 * 2^l + 3 rows"""
    r, out = "row band", []
    for l in range(LEVELS):
        for lr in range(max(l - 1, 0), min(l + 1, LEVELS - 1) + 1):
            rad = 2.0 * 2 ** lr
            lo_v, hi_v = up(100.0), down(101.0)
            assert np.floor(lo_v) == np.floor(hi_v) == 100.0
            assert np.floor(down(101.0 + rad) - rad) == 100.0 and np.floor((101.0 + rad) - rad) == 101.0
            assert np.ceil(up(99.0 - rad) + rad) == 100.0 and np.ceil((99.0 - rad) + rad) == 99.0
            for name, vl, vr, ok in (("floor(vR-r)==floor(vL)", lo_v, down(101.0 + rad), True), ("floor(vR-r) one step up", lo_v, 101.0 + rad, False),
                                     ("ceil(vR+r)==floor(vL)", hi_v, up(99.0 - rad), True), ("ceil(vR+r) one step down", hi_v, 99.0 - rad, False)):
                out.append(depth(r, "l=%d lr=%d %s" % (l, lr, name), [(200.0, vl, l, 0)], [(180.0, vr, lr, 0)],
                                 dict(flat(EDGE if ok else NO_CANDIDATE, int(ok)), best_idx=[0 if ok else -1])))
    return out


def _column_cases():
    r, out = "column range", []
    for tag, prm, lo, hi in (("window 8.25..64", dict(min_disparity=8.25, max_disparity=64.0), 236.5, 292.25),
                             ("max_disparity 0 = fx", dict(), 44.5, 300.5)):
        assert 300.5 - (prm.get("max_disparity") or FX) == lo and 300.5 - prm.get("min_disparity", 0.0) == hi
        for name, ur, ok in (("uR==uL-minD", hi, True), ("one step right of it", up(hi), False), ("uR==uL-maxD", lo, True),
                             ("one step left of it", down(lo), False)):
            out.append(depth(r, "%s %s" % (tag, name), [(300.5, 100.0, 0, 0)], [(ur, 100.0, 0, 0)],
                             dict(flat(EDGE if ok else NO_CANDIDATE, int(ok)), best_idx=[0 if ok else -1]), **prm))
    return out


def _th_dist_cases():
    r, out = "th_dist", []
    for th, d, st in ((75, 75, DESCRIPTOR), (75, 74, EDGE), (0, 0, DESCRIPTOR), (256, 256, DESCRIPTOR), (256, 255, EDGE), (1, 0, EDGE), (1, 1, DESCRIPTOR)):
        out.append(depth(r, "%d at %d" % (d, th), [(200.0, 100.0, 0, 0)], [(180.0, 100.0, 0, d)], dict(flat(st), best_idx=[0], best_dist=[d]), th_dist=th))
    return out


def _tie_cases():
    """row 6: every right keypoint is a candidate 200 bits away unless said otherwise; th_dist 256 lets the search go on"""
    r, out = "tie to the smallest j", []

    def one(name, n_r, special, best, dist, n_cand=None):
        right = [(180.0, 100.0, 0, 200)] * n_r
        for j, e in special.items():
            right[j] = e
        out.append(depth(r, name, [(200.0, 100.0, 0, 0)], right, dict(flat(EDGE, n_r if n_cand is None else n_cand), best_idx=[best], best_dist=[dist]),
                         th_dist=256))
    near = (180.0, 100.0, 0, 10)
    one("j and j+64", 130, {3: near, 67: near}, 3, 10)
    one("63 and 64", 130, {63: near, 64: near}, 63, 10)
    one("all equal", 130, {}, 0, 200)
    one("the best is the last of 65", 65, {64: near}, 64, 10)
    one("the best is the last of 257", 257, {256: near}, 256, 10)
    one("a nearer one of a refused level", 2, {0: (180.0, 100.0, 2, 0), 1: near}, 1, 10, 1)
    one("a nearer one of a refused row", 2, {0: (180.0, 103.0, 0, 0), 1: near}, 1, 10, 1)
    one("a nearer one of a refused column", 2, {0: (up(200.0), 100.0, 0, 0), 1: near}, 1, 10, 1)
    return out


def _rounding_and_border_cases():
    """rows 7 and 8 over the zero pictures: BORDER (sads -1) against EDGE (sads 0).  su == W cannot pass: uR <= uL gives sr <= su, and
    sr - 10 >= 0 fails first; both sides of that limit are BORDER"""
    out = []
    for l in range(LEVELS):
        s, wl, hl = float(2 ** l), WIDTH >> l, HEIGHT >> l
        mid_u, mid_v, mid_r, far_r = s * (wl // 2), s * (hl // 2), s * 20.0, s * (wl - 30)      # far_r: within fx = 256 of the last columns

        def one(row, name, ul, vl, ur, st):
            out.append(depth(row, "level %d %s" % (l, name), [(ul, vl, l, 0)], [(ur, vl, l, 0)], dict(flat(st), best_idx=[0])))
        half = [("su on the half", s * (wl - 5.5), mid_v, far_r, BORDER), ("su one step below the half", down(s * (wl - 5.5)), mid_v, far_r, EDGE),
                ("sv on the half", mid_u, s * 4.5, mid_r, EDGE), ("sv one step below the half", mid_u, down(s * 4.5), mid_r, BORDER),
                ("sr on the half", mid_u, mid_v, s * 9.5, EDGE), ("sr one step below the half", mid_u, mid_v, down(s * 9.5), BORDER)]
        for a in half:
            assert np.floor(s * (wl - 5.5) / s + 0.5) == wl - 5 and np.floor(down(s * (wl - 5.5)) / s + 0.5) == wl - 6
            assert np.floor(s * 4.5 / s + 0.5) == 5 and np.floor(down(s * 4.5) / s + 0.5) == 4 and np.floor(down(s * 9.5) / s + 0.5) == 9
            one("rounding", *a)
        if l == 2:
            continue
        for a in (("su==W", s * 5, mid_v, s * 5, BORDER), ("su==W-1", s * 4, mid_v, s * 4, BORDER),
                  ("su==Wl-W-1", s * (wl - 6), mid_v, far_r, EDGE), ("su==Wl-W", s * (wl - 5), mid_v, far_r, BORDER),
                  ("sv==W", mid_u, s * 5, mid_r, EDGE), ("sv==W-1", mid_u, s * 4, mid_r, BORDER),
                  ("sv==Hl-W-1", mid_u, s * (hl - 6), mid_r, EDGE), ("sv==Hl-W", mid_u, s * (hl - 5), mid_r, BORDER),
                  ("sr-10==0", mid_u, mid_v, s * 10, EDGE), ("sr-10==-1", mid_u, mid_v, s * 9, BORDER),
                  ("sr+10==Wl-1", s * (wl - 8), mid_v, s * (wl - 11), EDGE), ("sr+10==Wl", s * (wl - 8), mid_v, s * (wl - 10), BORDER)):
            one("border", *a)
    return out


# ---- the designed right picture of level 0 -----------------------------------------------------------------------------------------------------
# A strip is a right keypoint at (sr, sv) with a designed column of sums D[0..10].  The left picture is zero and row sv of the right one is
# zero on columns sr - 5 .. sr + 5, so D[q] is the sum of the marked values inside window q (columns sr - 10 + q .. sr + q, rows sv - 5 ..
# sv + 5).  A pixel on column sr - 10 + j is inside the windows 0 .. j, one on column sr + i inside the windows i .. 10, one on column sr
# inside all.  With m the FIRST minimum of D: the base D[m] goes on column sr (rows sv -+ 2 .. 5, at most 255 each), D[j] - D[j + 1] on
# column sr - 10 + j of row sv - 1 for j < m, D[i] - D[i - 1] on column sr + i of row sv + 1 for i > m.
STRIPS = collections.OrderedDict([
    ("k=-L", [5, 10, 20, 30, 40, 50, 60, 70, 80, 90, 100]),
    ("k=+L", [100, 90, 80, 70, 60, 50, 40, 30, 20, 10, 5]),
    ("k=-(L-1)", [20, 5, 10, 20, 30, 40, 50, 60, 70, 80, 90]),
    ("k=+(L-1)", [90, 80, 70, 60, 50, 40, 30, 20, 10, 5, 20]),
    ("plateau of three", [50, 40, 5, 5, 5, 30, 40, 50, 60, 70, 80]),
    ("plateau from column 0", [5, 5, 20, 30, 40, 50, 60, 70, 80, 90, 100]),
    ("d3==d2", [70, 60, 50, 40, 30, 10, 10, 40, 50, 60, 70]),
    ("d1==d3", [70, 60, 50, 40, 30, 10, 30, 40, 50, 60, 70]),
    ("delta=+1/4", [70, 60, 50, 40, 30, 0, 10, 40, 50, 60, 70]),
    ("delta=-1/4", [70, 60, 50, 40, 10, 0, 30, 40, 50, 60, 70]),
    ("delta=3/22", [60, 50, 40, 30, 20, 12, 5, 9, 20, 30, 40]),
    ("k=+1", [60, 50, 40, 30, 20, 12, 5, 12, 20, 30, 40]),
    ("k=-1", [40, 30, 20, 12, 5, 12, 20, 30, 40, 50, 60])] +
    [("sad %d" % v, [v + 10 * abs(q - 5) for q in range(11)]) for v in (0, 1, 3, 5, 7, 10, 21, 22, 30, 257, 272, 288, 600, 700, 261, 517, 1029, 1285)])
STRIP_NAMES = list(STRIPS)
assert len(STRIP_NAMES) <= 42


def strip_at(name):
    """(sr, sv) of a strip: a grid of three columns and fourteen rows, 80 and 16 apart"""
    t = STRIP_NAMES.index(name)
    return 40 + 80 * (t % 3), 16 + 16 * (t // 3)


def strip_desc(name):
    """the strip's own descriptor: 32 equal bytes, at least 32 bits from every other strip's"""
    return np.full(32, STRIP_NAMES.index(name) + 1, np.uint8)


def designed_level0():
    img = np.zeros((HEIGHT, WIDTH), np.uint8)
    for name, D in STRIPS.items():
        sr, sv = strip_at(name)
        m = int(np.argmin(D))
        assert all(D[j] >= D[j + 1] for j in range(m)) and all(D[i] >= D[i - 1] for i in range(m + 1, 11))
        base = D[m]
        for dy in (-2, 2, -3, 3, -4, 4, -5, 5):
            img[sv + dy, sr] = min(base, 255)
            base -= min(base, 255)
        assert base == 0
        for j in range(m):
            assert D[j] - D[j + 1] <= 255
            img[sv - 1, sr - 10 + j] = D[j] - D[j + 1]
        for i in range(m + 1, 11):
            assert D[i] - D[i - 1] <= 255
            img[sv + 1, sr + i] = D[i] - D[i - 1]
        assert not img[sv, sr - 5:sr + 6].any()
    return img


# ---- the designed right picture of level 1 -----------------------------------------------------------------------------------------------------
# The pyramid is pyrDown: separable [1 4 6 4 1], (sum + 128) >> 8.  One level-0 pixel of 255 at (2 r, 2 c) becomes at level 1 the blob
# [1 6 1; 6 36 6; 1 6 1] around (r, c): (36 * 255 + 128) >> 8 = 36, (6 * 255 + 128) >> 8 = 6, (255 + 128) >> 8 = 1; its columns sum to 8,
# 48, 8.  A blob on column sr - 6 adds [64 64 64 64 56 8 0 0 0 0 0] to D, one on sr + 6 the mirror image, one on sr + 7 [0 0 0 0 0 0 8 56
# 64 64 64], one on sr - 7 its mirror image.  Blobs whose columns reach sr - 5 .. sr + 5 stay off row sv.
BLOBS = collections.OrderedDict([      # name -> (sv, blobs (dr, dc) relative to (sv, sr), D, delta)
    ("d1==d3", (20, [(3, -6), (3, 6)], [64, 64, 64, 64, 56, 16, 56, 64, 64, 64, 64], 0.0)),
    ("d3==d2", (45, [(3, -6), (3, 7)], [64, 64, 64, 64, 56, 8, 8, 56, 64, 64, 64], 0.5)),
    ("delta=+1/4", (70, [(3, -6), (-4, 7), (0, 7), (4, 7)], [64, 64, 64, 64, 56, 8, 24, 168, 192, 192, 192], 0.25)),
    ("delta=-1/4", (95, [(-4, -7), (0, -7), (4, -7), (3, 6)], [192, 192, 192, 168, 24, 8, 56, 64, 64, 64, 64], -0.25))])
BLOB_SR = 80


def designed_level1():
    img = np.zeros((HEIGHT, WIDTH), np.uint8)
    for sv, blobs, _, _ in BLOBS.values():
        for dr, dc in blobs:
            img[2 * (sv + dr), 2 * (BLOB_SR + dc)] = 255
    return img


def pictures():
    """name -> the level-0 right picture.  The left picture is always "zero" """
    return collections.OrderedDict([("zero", np.zeros((HEIGHT, WIDTH), np.uint8)), ("level0", designed_level0()), ("level1", designed_level1())])


def all_strip_keypoints():
    return [(float(strip_at(n)[0]), float(strip_at(n)[1]), 0, strip_desc(n)) for n in STRIP_NAMES]


def strip_case(row, name, strip, status, k=None, delta=0.0, ul=None, extra=None, **params):
    """one left keypoint on a strip of the level-0 picture, 20 columns right of it unless ul is given.  OK: u_right = (sr + k) + delta,
    depth = bf / (uL - u_right), sad = D[k + 5]"""
    sr, sv = strip_at(strip)
    D = STRIPS[strip]
    ul = float(sr + 20) if ul is None else ul
    exp = dict(status=[status], best_idx=[STRIP_NAMES.index(strip)], best_dist=[0], sads=[D], right_idx=[-1], sad=[-1], u_right=[-1.0], depth=[-1.0])
    if status == S_OK:
        ur = float(sr + k) + delta
        exp.update(right_idx=[STRIP_NAMES.index(strip)], sad=[D[k + 5]], u_right=[ur], depth=[BF / (ul - ur) if extra is None else None])
    exp.update(extra or {})
    return depth(row, name, [(ul, float(sv), 0, strip_desc(strip))], all_strip_keypoints(), exp, right="level0", **params)


def _edge_cases():
    r = "k=+-L"
    return [strip_case(r, "k=-L", "k=-L", EDGE), strip_case(r, "k=+L", "k=+L", EDGE),
            strip_case(r, "k=-(L-1)", "k=-(L-1)", S_OK, -4, 0.25), strip_case(r, "k=+(L-1)", "k=+(L-1)", S_OK, 4, -0.25),
            strip_case(r, "a plateau takes its first column", "plateau of three", S_OK, -3, 0.5),
            strip_case(r, "a plateau from column 0", "plateau from column 0", EDGE)]


def _delta_cases():
    r = "delta"
    out = [strip_case(r, "level 0 d3==d2", "d3==d2", S_OK, 0, 0.5), strip_case(r, "level 0 d1==d3", "d1==d3", S_OK, 0, 0.0),
           strip_case(r, "level 0 +1/4", "delta=+1/4", S_OK, 0, 0.25), strip_case(r, "level 0 -1/4", "delta=-1/4", S_OK, 0, -0.25),
           strip_case(r, "level 0 3/22", "delta=3/22", S_OK, 1, 3.0 / 22.0)]
    right = [(2.0 * BLOB_SR, 2.0 * b[0], 1, t + 1) for t, b in enumerate(BLOBS.values())]
    for t, (name, (sv, _, D, delta)) in enumerate(BLOBS.items()):
        ul, ur = 2.0 * (BLOB_SR + 10), 2.0 * (float(BLOB_SR) + delta)
        out.append(depth(r, "level 1 " + name, [(ul, 2.0 * sv, 1, t + 1)], right, dict(
            status=[S_OK], best_idx=[t], best_dist=[0], sads=[D], right_idx=[t], sad=[D[5]], u_right=[ur], depth=[BF / (ul - ur)]), right="level1"))
    return out


def _disparity_cases():
    """row 11.  The strip "k=+1" fits u_right = sr + 1, "k=-1" sr - 1, both with delta 0, so the fitted disparity differs from the one the
    candidate filter saw"""
    r = "disparity"
    a, b = float(strip_at("k=+1")[0]), float(strip_at("k=-1")[0])
    assert down(a + 16.0) - (a + 1.0) < 15.0 == (a + 16.0) - (a + 1.0) and down(b + 14.0) - (b - 1.0) < 15.0 and down(a + 1.0) - (a + 1.0) < 0.0
    return [strip_case(r, "disp==minD", "k=+1", S_OK, 1, ul=a + 16.0, min_disparity=15.0),
            strip_case(r, "disp one step below minD", "k=+1", DISPARITY, ul=down(a + 16.0), min_disparity=15.0),
            strip_case(r, "disp==maxD", "k=-1", DISPARITY, ul=b + 14.0, max_disparity=15.0),
            strip_case(r, "disp one step below maxD", "k=-1", S_OK, -1, ul=down(b + 14.0), max_disparity=15.0),
            strip_case(r, "disp==0", "k=+1", S_OK, 1, ul=a + 1.0, extra=dict(u_right=[(a + 1.0) - 0.01], depth=[BF / 0.01])),
            strip_case(r, "disp the smallest negative", "k=+1", DISPARITY, ul=down(a + 1.0))]


def median_case(name, sads, note=None):
    """left keypoints on the strips "sad v" in the order of `sads` (None: a keypoint without a candidate, which is not counted); the
    literal statuses follow from the rule: med = element m / 2 of the sorted values, MEDIAN iff 10 sad > 21 med"""
    left, st, ri, sd, ur, dp = [], [], [], [], [], []
    values = sorted(v for v in sads if v is not None)
    med = values[len(values) // 2] if values else None
    for v in sads:
        if v is None:
            left.append((10.0, 232.0, 0, 0))
            st.append(NO_CANDIDATE), ri.append(-1), sd.append(-1), ur.append(-1.0), dp.append(-1.0)
            continue
        n = "sad %d" % v
        sr, sv = strip_at(n)
        left.append((sr + 20.0, float(sv), 0, strip_desc(n)))
        out = 10 * v > 21 * med
        st.append(MEDIAN if out else S_OK), ri.append(STRIP_NAMES.index(n)), sd.append(v)
        ur.append(-1.0 if out else float(sr)), dp.append(-1.0 if out else BF / 20.0)
    counts = [st.count(k) for k in range(7)]
    exp = dict(status=st, right_idx=ri, sad=sd, u_right=ur, depth=dp, counts=counts)
    if note is not None:
        assert [s for s, v in zip(st, sads) if v is not None] == note, (name, st)
    return depth("median", name, left, all_strip_keypoints(), exp, right="level0")


def _median_cases():
    o, m = S_OK, MEDIAN
    big = [None if i % 3 == 2 else (10 if i - i // 3 < 131 else 21 if i - i // 3 < 200 else 22) for i in range(390)]      # i - i // 3: its rank among the OK ones
    assert sum(v is not None for v in big) == 260 and sorted(v for v in big if v is not None)[130] == 10 != sorted(v for v in big if v is not None)[131]
    return [median_case("m=1", [7], [o]), median_case("m=1, sad 0", [0], [o]),
            median_case("m=2", [10, 22], [o, o]), median_case("m=2, the larger first", [22, 10], [o, o]),
            median_case("10 sad == 21 med", [10, 10, 10, 21, 22], [o, o, o, o, m]),
            median_case("even m", [22, 10, 22, 10], [o, o, o, o]), median_case("even m, med below", [5, 10, 10, 10, 21, 22], [o, o, o, o, o, m]),
            median_case("copies straddle m/2", [30, 10, 10, 3, 10, 10], [m, o, o, o, o, o]),
            median_case("med = 0", [0, 5, 0, 1, 0], [o, m, o, m, o]),
            median_case("high bytes differ", [1285, 517, 5, 1029, 261], [m, o, o, o, o]),
            median_case("low bytes differ", [700, 288, 257, 600, 272], [m, o, o, o, o]),
            median_case("no OK keypoint", [None, None]),
            median_case("260 OK keypoints among 390", big)]


DEPTH_ROWS = ("uL-minD", "level gate", "row band", "column range", "th_dist", "tie to the smallest j", "rounding", "border", "k=+-L", "delta",
              "disparity", "median")
_depths = None


def depth_cases():
    global _depths
    if _depths is None:
        out = (_step1_cases() + _level_cases() + _band_cases() + _column_cases() + _th_dist_cases() + _tie_cases() + _rounding_and_border_cases() +
               _edge_cases() + _delta_cases() + _disparity_cases() + _median_cases())
        assert len({c.name for c in out}) == len(out)
        _depths = out
    return list(_depths)


def depth_holds(case, out):
    """the names of the expected fields that `out` (stereo_match and stereo_candidates together) does not equal, bit for bit"""
    return [k for k, v in case.expected.items() if not equal_bits(out[k], v)]
