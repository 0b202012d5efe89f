"""Crafted cases that put one input ON each limit of the two stereo searches (ygz_slam_amd/csrc/strack.hip: k_strack_search and the host claim
walk; csrc/lfuse.hip: k_lfuse_search; DESIGN.md sections 12, 25, 26).  tests/test_search_limit_cases.py holds them to the restatements
(tests/strack_ref.c, tests/lfuse_ref.c) and to a numpy witness on the CPU, tests/test_gpu_search_limits.py runs them on the device.

Everything is built so that the compared quantities are exact in FP64, and "on the limit" means equality: intrinsics KX = (512, 512, 320,
240), the identity pose, points on or near the optical axis at power-of-two depths, baseline 0.125 (bf = 64), cos_near 0.75, r_near 2,
r_wide 4, chi2_mono 5, chi2_stereo 9.  One step beyond a limit is always np.nextafter.  No random number is drawn anywhere: every array is
written out.

A case is Case(name, kind, row, sets, problems, params, expected): kind "strack" or "lfuse", row the rule it is about, (sets, problems) one
point set and one problem in the form of strack_ref / lfuse_ref, params the parameter fields and "L" (the pyramid levels of the context),
expected the LITERAL outputs of the fields the case is about (lists, in the layout of the restatement's outputs).

base_cases() has every case in its smallest form.  all_cases() adds, for every base case, the same case with its keypoints moved to index
0, 7, 8, 255 and 256 (= n_kp - 1) of a list of 257 keypoints, padded with keypoints far outside every window (group of eight, tile of 256,
ragged end), and with its points moved to index 0, 63, 64 and 256 of a 257-point set whose other points pt_skip culls (wavefront, block,
ragged end).  pack() merges cases of one kind and one parameter set into calls of up to 64 problems over shared point sets."""
import collections

import numpy as np

KX = (512.0, 512.0, 320.0, 240.0)
W, H = 640, 480
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
FRAME, LOCAL = 0, 1
ST_PARAMS = dict(baseline=0.125, ratio=0.8, r_near=2.0, r_wide=4.0, cos_near=0.75, th_dist=100, check_orientation=1)
LF_PARAMS = dict(th=3.0, baseline=0.125, chi2_mono=5.0, chi2_stereo=9.0, th_dist=50, pad=0)
OPEN_GATE = 1048576.0                                   # a chi-square limit no case reaches: the gate of lfuse out of the way
KP_POSITIONS = (0, 7, 8, 255, 256)                      # 256 = n_kp - 1
PT_POSITIONS = (0, 63, 64, 256)
N_EMBED = 257
PER_POINT = ("match", "dist", "level", "pred_level", "reason", "outcome", "n_cand", "n_gated", "cand", "proj")
SKIPPED = dict(match=-1, dist=-1, level=-1, pred_level=-1, reason=1, outcome=-1, n_cand=0, n_gated=0, cand=[-1] * 8, proj=[0.0, 0.0, 0.0])
WIDE = (0.0, 0.0, 0.625)                                # a normal that passes the angle test (0.625 >= 0.5) and takes r_wide (0.625 <= 0.75)

Case = collections.namedtuple("Case", "name kind row sets problems params expected")


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def bits(d):
    """a descriptor with the first d bits set: Hamming distance d from the zero descriptor that every point carries"""
    return np.packbits(np.arange(256) < d)


def pt(pw=(0.0, 0.0, 4.0), level=0, dmax=4.0, normal=WIDE, angle=None, desc=0):
    return dict(pw=pw, level=level, dmax=dmax, normal=normal, angle=angle, desc=bits(desc))


def kp(px=(320.0, 240.0), level=0, dist=0, ur=-1.0, angle=0.0, taken=0):
    return dict(px=px, level=level, desc=bits(dist), ur=ur, angle=angle, taken=taken)


def make(kind, row, name, pts, kps, expected, th=None, direction=0, L=3, **fields):
    """one case from lists of pt() and kp().  kind "frame" / "local": strack with that mode; "lfuse": the fusion search (th is a parameter)"""
    angles = kind == "frame" and pts[0]["angle"] is not None
    s = dict(pw=np.array([p["pw"] for p in pts], np.float64).reshape(-1, 3), pt_desc=np.stack([p["desc"] for p in pts]))
    if kind == "frame":
        s["pt_level"] = np.array([p["level"] for p in pts], np.int32)
        if angles:
            s["pt_angle"] = np.array([p["angle"] for p in pts], np.float64)
    else:
        s["pt_dmax"] = np.array([p["dmax"] for p in pts], np.float64)
        s["pt_normal"] = np.array([p["normal"] for p in pts], np.float64).reshape(-1, 3)
    b = dict(T=np.array(IDENTITY), kp_px=np.array([k["px"] for k in kps], np.float64).reshape(-1, 2),
             kp_level=np.array([k["level"] for k in kps], np.int32), kp_desc=np.stack([k["desc"] for k in kps]),
             kp_ur=np.array([k["ur"] for k in kps], np.float64), set=0)
    if any(k["taken"] for k in kps):
        b["kp_taken"] = np.array([k["taken"] for k in kps], np.uint8)
    if kind == "lfuse":
        params = dict(LF_PARAMS, L=L, **fields)
        if th is not None:
            params["th"] = th
        expected = {("pred_level" if k == "level" else k): v for k, v in expected.items() if k in ("match", "dist", "level", "reason", "n_gated", "counts")}
    else:
        b.update(mode=FRAME if kind == "frame" else LOCAL, direction=direction, th=th if th is not None else (7.0 if kind == "frame" else 1.0))
        if angles:
            b["kp_angle"] = np.array([k["angle"] for k in kps], np.float64)
        params = dict(ST_PARAMS, L=L, **fields)
    return Case("%s/%s" % (kind, name), "lfuse" if kind == "lfuse" else "strack", row, [s], [b], params, expected)


def fields_of(case):
    """the parameter fields of a case without the pyramid levels: the keywords of strack_ref.search / lfuse_ref.search and of the bindings"""
    return {k: v for k, v in case.params.items() if k != "L"}


# ---- the rules both searches share ----------------------------------------------------------------------------------------------------------
def _projection_cases(kind):
    """step 2 (z > 0, the half-open image) for every kind; the distance range, the viewing angle and the predicted level for the two kinds
    that have them.  Every kept point has one keypoint on its projection with its descriptor and its level: match 0"""
    out = []

    def one(row, name, p, level, reason, px=(320.0, 240.0), **kw):
        lv = max(level, 0)
        p = dict(p, level=lv) if kind == "frame" else p
        exp = dict(reason=[reason], level=[level], match=[0 if reason == 0 else -1], dist=[0 if reason == 0 else -1])
        out.append(make(kind, row, name, [p], [kp(px, level=lv)], exp, **kw))
    one("z>0", "z=+0", pt((0.0, 0.0, 0.0)), -1, 2)
    one("z>0", "z=-0", pt((0.0, 0.0, -0.0)), -1, 2)
    one("z>0", "z=tiny", pt((0.0, 0.0, 2.0 ** -20), dmax=2.0 ** -20), 0, 0)
    # the points of test_points_on_the_limits (tests/test_gpu_projection.py): u = 0 and v = 0 kept, u = 640 and v = 480 culled
    for name, pw, px, reason in (("u=0", (-1.25, 0.0, 2.0), (0.0, 240.0), 0), ("u=640", (1.25, 0.0, 2.0), (639.5, 240.0), 3),
                                 ("v=0", (0.0, -0.9375, 2.0), (320.0, 0.0), 0), ("v=480", (0.0, 0.9375, 2.0), (320.0, 479.5), 3)):
        d = float(np.sqrt(pw[0] * pw[0] + pw[1] * pw[1] + pw[2] * pw[2]))
        one("image bounds", name, pt(pw, dmax=d, normal=pw), 0 if reason == 0 else -1, reason, px=px)
    if kind == "frame":
        return out
    hi, lo = 1.2 * 5.0, 0.8 * (5.0 / 4)                                 # dmax = 5, three levels: the range is [lo, hi]
    for name, z, level, reason in (("d=1.2dmax", hi, 0, 0), ("d>1.2dmax", up(hi), -1, 4), ("d=0.8dmin", lo, 2, 0), ("d<0.8dmin", down(lo), -1, 4)):
        one("distance range", name, pt((0.0, 0.0, z), dmax=5.0), level, reason)
    one("viewing angle", "c=0.5d", pt(normal=(0.0, 0.0, 0.5)), 0, 0)
    one("viewing angle", "c<0.5d", pt(normal=(0.0, 0.0, down(0.5))), -1, 5)
    for dmax, level in ((4.0, 0), (up(4.0), 1), (8.0, 1), (up(8.0), 2), (16.0, 2), (up(16.0), 2)):      # d = 4: dmax / d = 1, 2, 4 and one step above
        one("predicted level", "dmax=%r" % dmax, pt(dmax=dmax), level, 0)
    return out


def _window_cases(kind):
    """level 1, r = 14: a keypoint exactly r away on one side is no candidate, one step inside is"""
    out = []
    kw = dict(th=7.0, chi2_mono=OPEN_GATE, chi2_stereo=OPEN_GATE) if kind == "lfuse" else dict(th=7.0 if kind == "frame" else 1.75)
    p = pt(level=1, dmax=8.0)
    for side, on, inside in (("x+", (334.0, 240.0), (down(334.0), 240.0)), ("x-", (306.0, 240.0), (up(306.0), 240.0)),
                             ("y+", (320.0, 254.0), (320.0, down(254.0))), ("y-", (320.0, 226.0), (320.0, up(226.0)))):
        out.append(make(kind, "window", side + " on", [p], [kp(on, level=1)], dict(reason=[0], level=[1], match=[-1], n_cand=[0], n_gated=[0],
                                                                                  outcome=[1]), **kw))
        out.append(make(kind, "window", side + " inside", [p], [kp(inside, level=1)], dict(reason=[0], level=[1], match=[0], n_cand=[1],
                                                                                          n_gated=[0], outcome=[0]), **kw))
    # all four corners at once: on the limit in both coordinates
    out.append(make(kind, "window", "corners on", [p], [kp((334.0, 254.0), 1), kp((306.0, 226.0), 1), kp((334.0, 226.0), 1), kp((306.0, 254.0), 1)],
                    dict(match=[-1], n_cand=[0], outcome=[1]), **kw))
    return out


def _local_level_cases(kind):
    """five levels, d = 4, dmax = 16: pred = 2; keypoints of levels 0, 1, 2, 3 on the projection, 0, 2, 1 and 0 bits away"""
    kps = [kp(level=0, dist=0), kp(level=1, dist=2), kp(level=2, dist=1), kp(level=3, dist=0)]
    exp = dict(level=[2], match=[2], dist=[1], n_cand=[2], cand=[[2, 1, -1, -1, -1, -1, -1, -1]], outcome=[0])
    return [make(kind, "local level range", "pred=2 of 5", [pt(dmax=16.0)], kps, exp, L=5)]


def _stereo_sign_cases(kind):
    """a keypoint on the projection of a point with ur = 304: with a right column of 0.0 or -0.0 it is a stereo keypoint and the gate rejects
    it; with -1.0 or the double below zero it is mono and a candidate"""
    out = []
    for name, kur, stereo in (("ur=+0", 0.0, True), ("ur=-0", -0.0, True), ("ur=-1", -1.0, False), ("ur=below 0", down(0.0), False)):
        exp = dict(match=[-1 if stereo else 0], n_gated=[1 if stereo else 0], n_cand=[0 if stereo else 1], outcome=[1 if stereo else 0])
        out.append(make(kind, "stereo iff kp_ur >= 0", name, [pt()], [kp(ur=kur)], exp))
    return out


# ---- strack alone ----------------------------------------------------------------------------------------------------------------------------
def _radius_factor_cases():
    """c = 0.75 d takes r_wide (r = 4 at th 1): a keypoint 3 px off is a candidate; one step above takes r_near (r = 2): it is none"""
    k = [kp((323.0, 240.0))]
    return [make("local", "radius factor", "c=cos_near d", [pt(normal=(0.0, 0.0, 0.75))], k, dict(match=[0], n_cand=[1], outcome=[0])),
            make("local", "radius factor", "c>cos_near d", [pt(normal=(0.0, 0.0, up(0.75)))], k, dict(match=[-1], n_cand=[0], outcome=[1]))]


def _frame_level_cases():
    """five levels, one keypoint per level on the projection, all with the point's descriptor: the list is the level range in index order"""
    out = []
    want = {(2, -1): [0, 1, 2], (2, 0): [1, 2, 3], (2, 1): [2, 3, 4], (0, -1): [0], (0, 0): [0, 1], (0, 1): [0, 1, 2, 3, 4],
            (4, -1): [0, 1, 2, 3, 4], (4, 0): [3, 4], (4, 1): [4]}
    for (lvl, direction), lst in want.items():
        exp = dict(level=[lvl], n_cand=[len(lst)], cand=[lst + [-1] * (8 - len(lst))], match=[lst[0]], outcome=[0])
        out.append(make("frame", "frame level range", "lvl=%d dir=%+d" % (lvl, direction), [pt(level=lvl)], [kp(level=l) for l in range(5)], exp,
                        direction=direction, L=5))
    return out


def _gate_cases():
    """FRAME, level 1, th 7: r = 14, ur = 320 - 64 / 4 = 304.  The gate is closed: a column exactly r away survives"""
    out = []
    for name, kur, gated in (("ur+r", 318.0, 0), ("ur-r", 290.0, 0), ("above ur+r", up(318.0), 1), ("below ur-r", down(290.0), 1)):
        exp = dict(n_gated=[gated], n_cand=[1 - gated], match=[-1 if gated else 0], outcome=[1 if gated else 0], proj=[[320.0, 240.0, 304.0]])
        out.append(make("frame", "right-column gate", name, [pt(level=1)], [kp(level=1, ur=kur)], exp))
    # LOCAL: r = (1.75 * 4) * 2 = 14 as well
    for name, kur, gated in (("ur+r", 318.0, 0), ("above ur+r", up(318.0), 1), ("ur-r", 290.0, 0), ("below ur-r", down(290.0), 1)):
        exp = dict(n_gated=[gated], n_cand=[1 - gated], match=[-1 if gated else 0], outcome=[1 if gated else 0])
        out.append(make("local", "right-column gate", name, [pt(dmax=8.0)], [kp(level=1, ur=kur)], exp, th=1.75))
    return out


def _list_cases():
    """step 7: the survivors sorted by (distance, index), cut to eight, no distance threshold"""
    out = []
    first8 = list(range(8))
    out.append(make("frame", "sorted list", "nine equal", [pt()], [kp(dist=10) for _ in range(9)],
                    dict(cand=[first8], n_cand=[9], match=[0], dist=[10], counts=[[1, 1, 1, 0]])))
    out.append(make("frame", "sorted list", "the ninth is closer", [pt()], [kp(dist=10) for _ in range(8)] + [kp(dist=5)],
                    dict(cand=[[8] + first8[:7]], n_cand=[9], match=[8], dist=[5], counts=[[1, 1, 1, 0]])))
    out.append(make("frame", "sorted list", "the ninth ties", [pt()], [kp(dist=5)] + [kp(dist=10) for _ in range(7)] + [kp(dist=10)],
                    dict(cand=[first8], n_cand=[9], match=[0], dist=[5])))
    out.append(make("frame", "sorted list", "descending", [pt()], [kp(dist=90 - 10 * j) for j in range(9)],
                    dict(cand=[[8, 7, 6, 5, 4, 3, 2, 1]], n_cand=[9], match=[8], dist=[10])))
    out.append(make("frame", "sorted list", "a tie of two", [pt()], [kp(dist=30), kp(dist=30)],
                    dict(cand=[[0, 1] + [-1] * 6], n_cand=[2], match=[0], dist=[30])))
    out.append(make("frame", "sorted list", "a tie behind a closer one", [pt()], [kp(dist=30), kp(dist=30), kp(dist=29)],
                    dict(cand=[[2, 0, 1] + [-1] * 5], n_cand=[3], match=[2], dist=[29])))
    # 256 (every bit differs) is a valid key: it sorts behind 255 and is the match at th_dist 256
    out.append(make("frame", "sorted list", "256 behind 255", [pt()], [kp(dist=256), kp(dist=255)],
                    dict(cand=[[1, 0] + [-1] * 6], n_cand=[2], match=[1], dist=[255]), th_dist=256))
    out.append(make("frame", "sorted list", "256 in the list", [pt()], [kp(dist=256)],
                    dict(cand=[[0] + [-1] * 7], n_cand=[1], match=[-1], dist=[-1], outcome=[2])))
    return out


def _distance_cases():
    """step 8: dist(e1) > th_dist -> outcome 2.  LOCAL, both keypoints of level 0: (100, 125) also sits on the ratio limit 0.8 * 125 = 100"""
    two = lambda a, b: [kp(dist=a), kp(dist=b)]
    return [make("local", "th_dist", "(100,125) at 100", [pt()], two(100, 125), dict(match=[0], dist=[100], outcome=[0])),
            make("local", "th_dist", "(101,125) at 100", [pt()], two(101, 125), dict(match=[-1], dist=[-1], outcome=[2])),
            make("frame", "th_dist", "100 at 100", [pt()], [kp(dist=100)], dict(match=[0], dist=[100], outcome=[0])),
            make("frame", "th_dist", "101 at 100", [pt()], [kp(dist=101)], dict(match=[-1], dist=[-1], outcome=[2])),
            make("frame", "th_dist", "256 at 256", [pt()], [kp(dist=256)], dict(match=[0], dist=[256], outcome=[0]), th_dist=256),
            make("local", "th_dist", "256 at 256", [pt()], [kp(dist=256)], dict(match=[0], dist=[256], outcome=[0]), th_dist=256),
            make("frame", "th_dist", "0 at 0", [pt()], [kp(dist=0)], dict(match=[0], dist=[0], outcome=[0]), th_dist=0),
            make("frame", "th_dist", "1 at 0", [pt()], [kp(dist=1)], dict(match=[-1], dist=[-1], outcome=[2]), th_dist=0)]


def _ratio_cases():
    """step 8, LOCAL: outcome 3 iff e2 has e1's level and (double) d1 > ratio (double) d2.  Every pair (4k, 5k) at ratio 0.8 and (3k, 5k) at
    0.6 with 5k <= 256 sits ON the limit: in FP64 ratio * 5k rounds to 4k (3k) for every k, so none compares as greater -- matched"""
    out = []
    two = lambda a, b, lb=0: [kp(dist=a), kp(level=lb, dist=b)]
    for k in range(1, 52):
        out.append(make("local", "ratio", "(%d,%d) at 0.8" % (4 * k, 5 * k), [pt()], two(4 * k, 5 * k), dict(match=[0], dist=[4 * k], outcome=[0]),
                        th_dist=256))
        out.append(make("local", "ratio", "(%d,%d) at 0.8" % (4 * k + 1, 5 * k), [pt()], two(4 * k + 1, 5 * k), dict(match=[-1], dist=[-1], outcome=[3]),
                        th_dist=256))
        out.append(make("local", "ratio", "(%d,%d) at 0.6" % (3 * k, 5 * k), [pt()], two(3 * k, 5 * k), dict(match=[0], dist=[3 * k], outcome=[0]),
                        th_dist=256, ratio=0.6))
        out.append(make("local", "ratio", "(%d,%d) at 0.6" % (3 * k + 1, 5 * k), [pt()], two(3 * k + 1, 5 * k), dict(match=[-1], dist=[-1], outcome=[3]),
                        th_dist=256, ratio=0.6))
    # one step of the RATIO below 0.8: 4 > nextafter(0.8, 0) * 5 in FP64 (the product rounds below 4), while in float the ratio is 0.8f again
    out.append(make("local", "ratio", "(4,5) below 0.8", [pt()], two(4, 5), dict(match=[-1], outcome=[3]), ratio=down(0.8)))
    out.append(make("local", "ratio", "(4,5) above 0.8", [pt()], two(4, 5), dict(match=[0], outcome=[0]), ratio=up(0.8)))
    # the second entry on another level (pred = 1: levels 0 and 1 are searched): no ratio test
    out.append(make("local", "ratio", "(5,5) two levels", [pt(dmax=8.0)], two(5, 5, lb=1), dict(match=[0], dist=[5], outcome=[0], level=[1])))
    out.append(make("local", "ratio", "(5,5) one level", [pt(dmax=8.0)], two(5, 5), dict(match=[-1], dist=[-1], outcome=[3], level=[1])))
    # the second entry above th_dist still fires the rule: 100 > 0.8 * 110
    out.append(make("local", "ratio", "(100,110) at th_dist 100", [pt()], two(100, 110), dict(match=[-1], outcome=[3])))
    out.append(make("local", "ratio", "(100,126) at th_dist 100", [pt()], two(100, 126), dict(match=[0], dist=[100], outcome=[0])))
    # FRAME has no ratio test
    out.append(make("frame", "ratio", "(5,5) FRAME", [pt()], two(5, 5), dict(match=[0], dist=[5], outcome=[0])))
    return out


def _claim_cases():
    """step 8: e1, e2 are the first two entries NOT TAKEN"""
    out = []
    # two points on one pixel: the second one's best entry was claimed by the first
    out.append(make("local", "claim", "best claimed", [pt(), pt()], [kp(dist=0), kp(dist=20)],
                    dict(match=[0, 1], dist=[0, 20], outcome=[0, 0], cand=[[0, 1] + [-1] * 6] * 2, counts=[[2, 2, 0, 0]])))
    # a taken entry between e1 and e2.  Point 0 projects to u = 314 (r = 4: window (310, 318)) and sees keypoint 0 alone; point 1 on the axis
    # sees all three: its list is [1 (40), 0 (41), 2 (60)], keypoint 0 is taken, e2 is keypoint 2: 40 > 0.8 * 60 is false -> matched
    out.append(make("local", "claim", "taken between e1 and e2", [pt((-0.046875, 0.0, 4.0)), pt()],
                    [kp((317.0, 240.0), dist=41), kp((321.0, 240.0), dist=40), kp((322.0, 240.0), dist=60)],
                    dict(match=[0, 1], dist=[41, 40], outcome=[0, 0], n_cand=[1, 3], cand=[[0] + [-1] * 7, [1, 0, 2] + [-1] * 5],
                         proj=[[314.0, 240.0, 298.0], [320.0, 240.0, 304.0]])))
    # the same with the taken entry first: e1 = 1 (41), e2 = 2 (60)
    out.append(make("local", "claim", "taken before e1", [pt((-0.046875, 0.0, 4.0)), pt()],
                    [kp((317.0, 240.0), dist=40), kp((321.0, 240.0), dist=41), kp((322.0, 240.0), dist=51)],
                    dict(match=[0, -1], dist=[40, -1], outcome=[0, 3], cand=[[0] + [-1] * 7, [0, 1, 2] + [-1] * 5])))
    # nine points on one pixel, nine keypoints 1 .. 9 bits away: points 0 .. 7 claim keypoints 0 .. 7; the last one's list holds those eight
    # and not the free ninth -> outcome 1 (the truncation the spec accepts)
    out.append(make("frame", "claim", "eight taken, a ninth free", [pt() for _ in range(9)], [kp(dist=j + 1) for j in range(9)],
                    dict(match=list(range(8)) + [-1], outcome=[0] * 8 + [1], n_cand=[9] * 9, cand=[list(range(8))] * 9, counts=[[8, 9, 9, 0]])))
    # kp_taken preset: the keypoint is no candidate at all (step 5)
    out.append(make("frame", "claim", "kp_taken preset", [pt()], [kp(dist=0, taken=1), kp(dist=10)],
                    dict(match=[1], dist=[10], n_cand=[1], cand=[[1] + [-1] * 7], outcome=[0])))
    out.append(make("local", "claim", "kp_taken preset, ratio", [pt()], [kp(dist=9), kp(dist=10, taken=1), kp(dist=20)],
                    dict(match=[0], dist=[9], n_cand=[2], cand=[[0, 2] + [-1] * 6], outcome=[0])))
    return out


def rotation_set(hist, seed):
    """pt_angle, kp_angle [n] whose differences fall into the prescribed bins: orientation_problem of tests/bow_cases.py with as many rows as
    matches, row i matched to keypoint i"""
    import bow_cases as bc
    n = int(np.sum(hist))
    p = bc.orientation_problem(hist, n, n, seed)
    assert (p["m"] >= 0).all()
    return p["a1"], p["a2"][p["m"]]


def _grid(n):
    """n points at depth 4 whose projections are 64 px apart (exact: x = k / 2 -> u = 320 + 64 k), far more than a window of r = 7"""
    assert n <= 63
    return [((k % 9 - 4) * 0.5, (k // 9 - 3) * 0.5, 4.0) for k in range(n)]


def _orientation_cases():
    """step 9, FRAME with angles.  One point, one keypoint: the histogram has one entry, in the bin of the difference.  Several points, each
    with its own keypoint on its projection: the three maxima and the 0.1 rule decide which matches stay"""
    import bow_cases as bc
    out = []
    for diff, b in ((14.99, 0), (15.0, 1), (15.01, 1), (344.99, 11), (345.0, 12), (-0.0, 0), (-15.0, 12), (44.99, 1), (45.0, 2), (359.99, 12)):
        rot = [0] * 30 + [b, -1, -1]
        rot[b] = 1
        out.append(make("frame", "orientation", "diff=%r" % diff, [pt(angle=diff)], [kp(angle=0.0)], dict(match=[0], outcome=[0], rot=[rot])))
    out.append(make("frame", "orientation", "diff=15 from 350", [pt(angle=5.0)], [kp(angle=350.0)],
                    dict(match=[0], rot=[[0, 1] + [0] * 28 + [1, -1, -1]])))
    for name, hist, ind, kept in (("10 1", bc.hist30(b3=10, b8=1), [3, 8, -1], 11), ("20 2", bc.hist30(b5=20, b6=2), [5, 6, -1], 22),
                                  ("30 2", bc.hist30(b2=30, b9=2), [2, -1, -1], 30), ("10 1 1", bc.hist30(b3=10, b0=1, b8=1), [3, 0, 8], 12),
                                  ("20 2 1", bc.hist30(b5=20, b6=2, b7=1), [5, 6, -1], 22), ("5 5 5 5", bc.hist30(b2=5, b5=5, b7=5, b9=5), [2, 5, 7], 15)):
        n = int(hist.sum())
        a1, a2 = rotation_set(hist, 100 + n)
        pw = _grid(n)
        pts = [pt(pw[i], angle=float(a1[i])) for i in range(n)]
        kps = [kp((320.0 + 128.0 * pw[i][0], 240.0 + 128.0 * pw[i][1]), angle=float(a2[i])) for i in range(n)]
        out.append(make("frame", "orientation", "histogram " + name, pts, kps,
                        dict(rot=[[int(x) for x in hist] + ind], counts=[[kept, n, 0, n - kept]], n_cand=[1] * n)))
    return out


# ---- lfuse alone -----------------------------------------------------------------------------------------------------------------------------
def _chi2_cases():
    """step 7b: out iff e2 > chi2 * 4^level of the KEYPOINT's level.  th 3: r = 3 at level 0, 6 at level 1; ur = 304"""
    out = []
    one = lambda name, p, k, gated, **kw: out.append(make("lfuse", "chi-square gate", name, [p], [k], dict(
        match=[-1 if gated else 0], n_gated=[gated], reason=[0]), **kw))
    one("mono e2=5", pt(), kp((321.0, 242.0)), 0)
    one("mono e2>5", pt(), kp((321.0, up(242.0))), 1)
    one("mono e2=5 mirrored", pt(), kp((318.0, 239.0)), 0)
    one("mono e2>5 mirrored", pt(), kp((down(318.0), 239.0)), 1)
    one("stereo e2=9", pt(), kp((321.0, 242.0), ur=302.0), 0)
    one("stereo e2>9 in v", pt(), kp((321.0, up(242.0)), ur=302.0), 1)
    one("stereo e2>9 in ur", pt(), kp((321.0, 242.0), ur=down(302.0)), 1)
    one("stereo e2=9 column above", pt(), kp((321.0, 242.0), ur=306.0), 0)
    one("stereo e2>9 column above", pt(), kp((321.0, 242.0), ur=up(306.0)), 1)
    one("level 1 keypoint e2=20", pt(dmax=8.0), kp((322.0, 244.0), level=1), 0)
    one("level 1 keypoint e2>20", pt(dmax=8.0), kp((322.0, up(244.0)), level=1), 1)
    one("level 0 keypoint e2=20 at pred 1", pt(dmax=8.0), kp((322.0, 244.0), level=0), 1)
    one("level 1 stereo e2=36", pt(dmax=8.0), kp((322.0, 244.0), level=1, ur=300.0), 0)
    one("level 1 stereo e2>36", pt(dmax=8.0), kp((322.0, 244.0), level=1, ur=down(300.0)), 1)
    return out


def _lfuse_distance_cases():
    """step 8: a match when the smallest distance is <= th_dist"""
    out = []
    for th_dist in (0, 50, 256):
        out.append(make("lfuse", "lfuse th_dist", "%d at %d" % (th_dist, th_dist), [pt()], [kp(dist=th_dist)],
                        dict(match=[0], dist=[th_dist], counts=[[1, 1]]), th_dist=th_dist))
        if th_dist < 256:
            out.append(make("lfuse", "lfuse th_dist", "%d at %d" % (th_dist + 1, th_dist), [pt()], [kp(dist=th_dist + 1)],
                            dict(match=[-1], dist=[-1], counts=[[0, 1]]), th_dist=th_dist))
    # the smallest (distance, index); one above th_dist is not replaced by a farther one within it -- there is none -- and ties keep the index
    out.append(make("lfuse", "lfuse th_dist", "a tie of two", [pt()], [kp(dist=50), kp(dist=50)], dict(match=[0], dist=[50])))
    out.append(make("lfuse", "lfuse th_dist", "255 before 256", [pt()], [kp(dist=256), kp(dist=255)], dict(match=[1], dist=[255]), th_dist=256))
    return out


# ---- the lists -------------------------------------------------------------------------------------------------------------------------------
_base = None


def base_cases():
    global _base
    if _base is None:
        out = []
        for kind in ("lfuse", "local", "frame"):
            out += _projection_cases(kind) + _window_cases(kind) + _stereo_sign_cases(kind)
        out += _local_level_cases("lfuse") + _local_level_cases("local")
        out += _radius_factor_cases() + _frame_level_cases() + _gate_cases() + _list_cases() + _distance_cases() + _ratio_cases() + _claim_cases()
        out += _orientation_cases() + _chi2_cases() + _lfuse_distance_cases()
        assert len({c.name for c in out}) == len(out)
        _base = out
    return list(_base)


def n_points(case):
    return len(case.sets[0]["pt_desc"])


def n_keypoints(case):
    return len(case.problems[0]["kp_level"])


def keypoints_at(case, pos):
    """the case with its keypoints, in their order, at indices start .. of a list of N_EMBED; the others lie at (8, 8), outside every window"""
    k = n_keypoints(case)
    start = min(pos, N_EMBED - k)
    b = dict(case.problems[0])
    fill = dict(kp_px=8.0, kp_level=0, kp_desc=0, kp_ur=-1.0, kp_angle=0.0, kp_taken=0)
    for name, v in fill.items():
        if name in b:
            a = np.asarray(b[name])
            full = np.full((N_EMBED,) + a.shape[1:], v, a.dtype)
            full[start:start + k] = a
            b[name] = full
    exp = dict(case.expected)
    for f in ("match", "cand"):
        if f in exp:
            a = np.asarray(exp[f])
            exp[f] = np.where(a >= 0, a + start, a).tolist()
    return case._replace(name="%s @kp%d" % (case.name, pos), problems=[b], expected=exp)


def points_at(case, pos):
    """the case with its points, in their order, at indices start .. of a set of N_EMBED points; pt_skip culls the others"""
    n = n_points(case)
    start = min(pos, N_EMBED - n)
    s = dict(case.sets[0])
    fill = dict(pw=(0.0, 0.0, 4.0), pt_desc=0, pt_level=0, pt_angle=0.0, pt_dmax=4.0, pt_normal=(0.0, 0.0, 1.0))
    for name, v in fill.items():
        if name in s:
            a = np.asarray(s[name])
            full = np.empty((N_EMBED,) + a.shape[1:], a.dtype)
            full[:] = v
            full[start:start + n] = a
            s[name] = full
    b = dict(case.problems[0])
    skip = np.ones(N_EMBED, np.uint8)
    skip[start:start + n] = 0
    b["pt_skip"] = skip
    exp = {}
    for f, v in case.expected.items():
        if f in PER_POINT:
            full = [SKIPPED[f]] * N_EMBED
            full[start:start + n] = v
            exp[f] = full
        else:
            exp[f] = v
    return case._replace(name="%s @pt%d" % (case.name, pos), sets=[s], problems=[b], expected=exp)


_all = None


def all_cases():
    global _all
    if _all is None:
        out = []
        for c in base_cases():
            out.append(c)
            out += [keypoints_at(c, p) for p in KP_POSITIONS]
            out += [points_at(c, p) for p in PT_POSITIONS]
        _all = out
    return list(_all)


def group_key(case):
    b, s = case.problems[0], case.sets[0]
    return (case.kind, b.get("mode", -1), "pt_angle" in s, tuple(sorted(case.params.items())))


def families(cases):
    """the cases that may share one call: one kind, one mode, one parameter set, one pyramid"""
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault(group_key(c), []).append(c)
    return list(out.values())


def pack(cases, max_problems=64, max_sets=8, max_points=N_EMBED):
    """one family as calls of up to max_problems problems over at most max_sets shared point sets of up to max_points points.  The cases
    with small sets come first: their sets are concatenated.  The cases whose set already has max_points points (points_at) are laid over one
    another where the points they do not skip do not collide.  Every problem skips the points of the other cases in its set.  Returns
    [(sets, problems, slots)], slots [(case, problem index, first point within the problem's set, its number of points)]"""
    calls, sets, problems, slots, members = [], [], [], [], []

    def live(c):
        skip = c.problems[0].get("pt_skip")
        return np.ones(n_points(c), bool) if skip is None else np.asarray(skip).reshape(-1) == 0

    def close_set():
        if not members:
            return
        keys = members[0][0].sets[0].keys()
        if members[0][2] is None:                                       # laid over one another
            merged = {k: np.array(members[0][0].sets[0][k]) for k in keys}
            for c, _, _ in members[1:]:
                for k in keys:
                    merged[k][live(c)] = np.asarray(c.sets[0][k])[live(c)]
        else:
            merged = {k: np.concatenate([np.asarray(c.sets[0][k]) for c, _, _ in members]) for k in keys}
        total = len(merged["pt_desc"])
        for c, q, at in members:
            at, n = at or 0, n_points(c)
            skip = np.ones(total, np.uint8)
            skip[at:at + n] = ~live(c)
            problems[q] = dict(problems[q], pt_skip=skip, set=len(sets))
            slots[q] = (c, q, at, n)
        sets.append(merged)
        del members[:]

    def close_call():
        close_set()
        if problems:
            calls.append((list(sets), list(problems), list(slots)))
        del sets[:], problems[:], slots[:]
    for c in sorted(cases, key=lambda c: n_points(c) >= max_points):      # stable: the small sets first
        assert len(c.sets) == 1 and len(c.problems) == 1
        if n_points(c) >= max_points:
            if members and (members[0][2] is not None or any((live(m) & live(c)).any() for m, _, _ in members)):
                close_set()
            at = None
        else:
            at = sum(n_points(m) for m, _, _ in members)
            if at + n_points(c) > max_points:
                close_set()
                at = 0
        if len(problems) >= max_problems or len(sets) >= max_sets:
            close_call()
            at = at and 0
        members.append((c, len(problems), at))
        problems.append(dict(c.problems[0]))
        slots.append(None)
    close_call()
    return calls


def slot_outputs(out, offsets, slot):
    """the outputs of a packed call that belong to one case, in the layout of the case alone"""
    c, q, at, n = slot
    o = int(offsets[q]) + at
    return {k: (v[o:o + n] if k in PER_POINT else v[q:q + 1]) for k, v in out.items() if k != "offsets"}


def holds(case, out):
    """the names of the expected fields that `out` (of the case alone, or slot_outputs) does not equal"""
    return [k for k, v in case.expected.items() if np.asarray(out[k]).tolist() != np.asarray(v).tolist()]
