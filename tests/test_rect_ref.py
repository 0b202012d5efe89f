"""The restatement of the stereo rectification (tests/rect_ref.c, the frozen spec of DESIGN.md section 23) held to a numpy witness written
another way -- Bouguet's construction through rotation vectors with sin and cos as cv::stereoRectify orders it, whole-array maps -- and to what
the model must do whatever its code: the invariants of the two rotations over 2000 random rigs, every refusal, R = I is the lens-only map, a
round trip through an analytic picture seen by the rig, and the stereo matcher's verdict on a textured pair before and after.  No device."""
import numpy as np
import pytest

import rect_ref as rr
import stereo_ref as sr
import undist_ref as ur
from test_undist_ref import CASES, analytic

W, H, D = rr.RIG_W, rr.RIG_H, rr.RIG_D


def rotation_vector(R):
    """the inverse of rr.rodrigues.  The angle is atan2(sin, cos) where OpenCV takes acos(cos): acos cannot tell an angle of 1e-9 from none"""
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.sqrt(a @ a)), 0.5 * (np.trace(R) - 1.0)
    if s == 0.0:
        return np.zeros(3)
    return a * (np.arctan2(s, c) / s)


def witness_rectify(R, T):
    """cv::stereoRectify's steps for a horizontal rig whose second camera is to the right"""
    r_r = rr.rodrigues(-0.5 * rotation_vector(R))
    t = r_r @ T
    uu = np.array([-1.0, 0.0, 0.0])
    ww = np.cross(t, uu)
    nw = float(np.sqrt(ww @ ww))
    if nw > 0.0:
        ww = ww * (np.arctan2(nw, abs(t[0])) / nw)
    wR = rr.rodrigues(ww)
    return wR @ r_r.T, wR @ r_r, float(np.sqrt(t @ t))


def random_rigs(n, seed):
    rng = np.random.default_rng(seed)
    scales = (0.0, 1e-9, 1e-3, 0.05, 0.3)
    for i in range(n):
        s = scales[i % len(scales)]
        axis = rng.normal(size=3)
        R = np.eye(3) if s == 0.0 else rr.rodrigues(axis / np.linalg.norm(axis) * s * rng.uniform(0.2, 1.0))
        T = np.array([-rng.uniform(0.05, 0.6), 0.02 * rng.normal(), 0.02 * rng.normal()])
        yield R, T


def test_rotations_over_random_rigs():
    worst = dict(orth=0.0, det=0.0, chain=0.0, base=0.0, wit=0.0)
    n = 0
    for R, T in random_rigs(2000, 7):
        got = rr.stereo_rectify(R, T)
        assert got is not None, (R, T)
        R1, R2, b = got
        for M in (R1, R2):
            worst["orth"] = max(worst["orth"], np.abs(M @ M.T - np.eye(3)).max())
            worst["det"] = max(worst["det"], abs(np.linalg.det(M) - 1.0))
        worst["chain"] = max(worst["chain"], np.abs(R2 @ R @ R1.T - np.eye(3)).max())
        worst["base"] = max(worst["base"], np.abs(R2 @ T - np.array([-b, 0.0, 0.0])).max() / b)
        w1, w2, wb = witness_rectify(R, T)
        worst["wit"] = max(worst["wit"], np.abs(R1 - w1).max(), np.abs(R2 - w2).max(), abs(b - wb))
        n += 1
    print("2000 rigs, worst: %s" % {k: "%.2e" % v for k, v in worst.items()})
    assert n == 2000
    assert worst["orth"] <= 1e-14 and worst["det"] <= 1e-14 and worst["chain"] <= 1e-14 and worst["base"] <= 1e-14, worst
    assert worst["wit"] <= 1e-12, worst


def test_the_rig():
    R1, R2, b = rr.stereo_rectify(rr.RIG_R, rr.RIG_T)
    assert abs(b - 0.110059075046) < 1e-12
    # R = I, T along -x: nothing to turn
    R1, R2, b = rr.stereo_rectify(np.eye(3), [-0.25, 0.0, 0.0])
    assert np.array_equal(R1, np.eye(3)) and np.array_equal(R2, np.eye(3)) and b == 0.25


def test_every_refusal():
    R, T = rr.RIG_R, rr.RIG_T
    assert rr.stereo_rectify(R, T) is not None
    for bad in (float("nan"), float("inf"), -float("inf")):
        for i in range(9):
            M = R.copy().reshape(9)
            M[i] = bad
            assert rr.stereo_rectify(M, T) is None, (i, bad)
        for i in range(3):
            t = T.copy()
            t[i] = bad
            assert rr.stereo_rectify(R, t) is None, (i, bad)
    assert rr.stereo_rectify(R, np.zeros(3)) is None                                   # b = 0
    assert rr.stereo_rectify(R * (1.0 + 1e-5), T) is None                              # not orthonormal: |R R^T - I| = 2e-5
    assert rr.stereo_rectify(R * (1.0 + 1e-8), T) is not None                          # inside the tolerance
    assert rr.stereo_rectify(np.diag([1.0, 1.0, -1.0]), T) is None                     # a reflection
    assert rr.stereo_rectify(np.zeros((3, 3)), T) is None
    assert rr.stereo_rectify(rr.rodrigues((0.0, 2.2, 0.0)), T) is None                 # 126 degrees apart: w <= 0.5
    assert rr.stereo_rectify(rr.rodrigues((0.0, 2.0, 0.0)), rr.rodrigues((0.0, 1.0, 0.0)) @ [-0.1, 0.0, 0.0]) is not None          # 115 degrees
    assert rr.stereo_rectify(rr.rodrigues((3.141592653589793, 0.0, 0.0)), T) is None   # half a turn: w = 0
    assert rr.stereo_rectify(np.eye(3), [0.11, 0.0, 0.0]) is None                      # the second camera is to the left
    assert rr.stereo_rectify(np.eye(3), [0.0, 0.1, 0.0]) is None                       # t[0] = 0
    assert rr.stereo_rectify(np.eye(3), [-0.01, 0.1, 0.0]) is None                     # a vertical rig
    assert rr.stereo_rectify(np.eye(3), [-0.01, 0.0, -0.1]) is None                    # one camera behind the other
    assert rr.stereo_rectify(np.eye(3), [-0.1, 0.1, 0.0]) is not None                  # |t[0]| = max(|t[1]|, |t[2]|) is still taken


def witness_map(w, h, p, cam):
    """(mx, my, front, qx, qy) by whole-array arithmetic in the spec's order"""
    fxd, fyd, cxd, cyd = cam
    l, r = p.lens, list(p.R)
    u, v = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        x0, y0 = (u - cxd) / fxd + 0.0 * v, (v - cyd) / fyd + 0.0 * u
        X, Y, Wd = (r[0] * x0 + r[3] * y0) + r[6], (r[1] * x0 + r[4] * y0) + r[7], (r[2] * x0 + r[5] * y0) + r[8]
        x, y = X / Wd, Y / Wd
        x2, y2 = x * x, y * y
        r2, xy2 = x2 + y2, 2.0 * (x * y)
        kr = 1.0 + ((l.k3 * r2 + l.k2) * r2 + l.k1) * r2
        xd = (x * kr + l.p1 * xy2) + l.p2 * (r2 + 2.0 * x2)
        yd = (y * kr + l.p1 * (r2 + 2.0 * y2)) + l.p2 * xy2
        mx, my = l.fx * xd + l.cx, l.fy * yd + l.cy
        front = Wd > 0.0
        inside = front & (mx > -2.0) & (mx < w + 1) & (my > -2.0) & (my < h + 1)
        qx = np.where(inside, np.rint(np.where(inside, mx, 0.0) * 32.0), rr.OUTSIDE).astype(np.int64).astype(np.int32)
        qy = np.where(inside, np.rint(np.where(inside, my, 0.0) * 32.0), rr.OUTSIDE).astype(np.int64).astype(np.int32)
    return mx, my, front, qx, qy


SMALL_CAMERAS = {(640, 480): ur.DEFAULT_CAMERA,
                 (150, 98): tuple(float(np.float32(v)) for v in (121.5, 121.6, 80.1, 48.7)),
                 (34, 32): tuple(float(np.float32(v)) for v in (30.0, 30.5, 17.1, 15.7))}
TILT_20 = rr.rodrigues((0.0, np.deg2rad(20.0), 0.0))


def map_cases(cam, border=0):
    """name -> rr.Params: the rig's two cameras scaled to the output camera, R = I behind the left lens, and a 20 degree tilt"""
    p0, p1, _ = rr.rig(cam, border)
    return {"left": p0, "right": p1, "identity": rr.params(p0.lens), "tilt": rr.params(p0.lens, TILT_20)}


@pytest.mark.parametrize("shape", list(SMALL_CAMERAS), ids=lambda s: "%dx%d" % s)
def test_map_equals_the_witness(shape):
    w, h = shape
    cam = SMALL_CAMERAS[shape]
    for name, p in map_cases(cam).items():
        qx, qy = rr.build_map(w, h, p, cam)
        mx, my, front = rr.map_real(w, h, p, cam)
        wmx, wmy, wfront, wx, wy = witness_map(w, h, p, cam)
        assert np.array_equal(qx, wx) and np.array_equal(qy, wy), name
        assert np.array_equal(mx, wmx) and np.array_equal(my, wmy) and np.array_equal(front, wfront), name
        assert np.array_equal(qx == rr.OUTSIDE, qy == rr.OUTSIDE)
        if name == "tilt":
            assert front.all() and (qx == rr.OUTSIDE).any() and (qx != rr.OUTSIDE).any()
        if name in ("left", "right") and shape == (640, 480):
            assert ((mx >= 0) & (mx <= w - 1) & (my >= 0) & (my <= h - 1)).all()          # every output pixel sees the picture
            box = rr.tile_boxes(qx, qy)
            assert box[..., 4].all() and (box[..., 2] * box[..., 3]).max() <= 2800         # no tile falls back
    # a camera turned away: W <= 0 is outside whatever the lens makes of it
    p = rr.params(map_cases(cam)["left"].lens, rr.rodrigues((0.0, np.deg2rad(100.0), 0.0)))
    qx, _ = rr.build_map(w, h, p, cam)
    _, _, front = rr.map_real(w, h, p, cam)
    assert not front.all() and (qx[~front] == rr.OUTSIDE).all()


@pytest.mark.parametrize("name", list(CASES))
def test_identity_rotation_is_the_lens_only_map(name):
    for (w, h), cam in SMALL_CAMERAS.items():
        lens = ur.params(cam, **CASES[name])
        ux, uy = ur.build_map(w, h, lens, cam)
        qx, qy = rr.build_map(w, h, rr.params(lens), cam)
        assert np.array_equal(qx, ux) and np.array_equal(qy, uy), (w, h)


def inside_of(p):
    mx, my, front = rr.map_real(W, H, p)
    return front & (mx >= 0) & (mx <= W - 1) & (my >= 0) & (my <= H - 1)


def test_round_trip_through_an_analytic_picture():
    """The analytic picture as the rig's two raw cameras see it (right: shifted by 20 columns), rectified: every output pixel whose source lies
    inside the raw picture matches its ideal picture to < 2 gray levels (section 18's budget of 1.69; the render is exact, so the rotation
    adds nothing), and the two rectified pictures are one picture 20 columns apart to 2 x 1.69 floored = 3 levels, which the raw ones are not."""
    p0, p1, _ = rr.rig()
    u, v = np.arange(W)[None, :] + np.zeros((H, 1)), np.arange(H)[:, None] + np.zeros((1, W))
    ideal = [analytic(u, v), analytic(u + D, v)]
    out, raw, inside = [], [], []
    for k, p in enumerate((p0, p1)):
        seen, res = rr.render_analytic(p, (lambda x, y, k=k: analytic(x + k * D, y)), W, H)
        ins = inside_of(p)
        mx, my, _ = rr.map_real(W, H, p)
        used = np.zeros((H, W), bool)
        sx, sy = np.floor(mx[ins]).astype(int), np.floor(my[ins]).astype(int)
        for dy in (0, 1):
            for dx in (0, 1):
                used[np.clip(sy + dy, 0, H - 1), np.clip(sx + dx, 0, W - 1)] = True
        assert res[used].max() <= 1e-15, res[used].max()
        got = rr.rectify(seen, p)
        err = np.abs(got.astype(np.float64) - ideal[k])[ins].max()
        print("round trip camera %d: %.3f gray levels over %.3f of the picture" % (k, err, ins.mean()))
        assert ins.mean() > 0.9 and err < 2.0, err
        out.append(got.astype(np.int64)); raw.append(seen.astype(np.int64)); inside.append(ins)
    both = inside[1][:, :W - D] & inside[0][:, D:]
    diff = np.abs(out[1][:, :W - D] - out[0][:, D:])[both].max()
    raw_diff = np.abs(raw[1][:, :W - D] - raw[0][:, D:])[both].max()
    print("rectified right against left 20 columns on: %d levels; the raw pair: %d" % (diff, raw_diff))
    assert both.mean() > 0.9 and diff <= 3
    assert raw_diff > 10 * 3                                                       # the raw pair fails the same comparison by far


def stereo_shares(o, left, right, baseline):
    """(share of the left keypoints that are OK, share of those with |disparity - 20| < 1)"""
    pl, pr = o.pyramid(left, 3), o.pyramid(right, 3)
    kl, kr = o.detect(pl), o.detect(pr)
    kl, kr = [sr.keypoints(np.stack([k["px"], k["py"]], 1), k["level"], k["desc"]) for k in (kl, kr)]
    m = sr.match(pl, pr, kl, kr, sr.params(baseline=baseline))
    ok = m["status"] == sr.OK
    n = len(kl["level"])
    good = np.abs(kl["px"][ok, 0] - m["u_right"][ok] - D) < 1.0
    return ok.sum() / float(n), (good.mean() if ok.any() else 0.0), n


@pytest.fixture(scope="module")
def shares(oracle):
    left, right, ideal_left, ideal_right = rr.textured_raw_pair()
    p0, p1, b = rr.rig()
    return {"ideal": stereo_shares(oracle, ideal_left, ideal_right, b),
            "raw": stereo_shares(oracle, left, right, b),
            "lens_only": stereo_shares(oracle, rr.rectify(left, rr.params(p0.lens)), rr.rectify(right, rr.params(p1.lens)), b),
            "rectified": stereo_shares(oracle, rr.rectify(left, p0), rr.rectify(right, p1), b)}


def test_the_matcher_before_and_after(shares):
    """The textured pair of the rig through the oracle's extractor and the stereo restatement.  The thresholds separate "rectified" from
    "not"; they are no performance claims."""
    for k, (ok, good, n) in shares.items():
        print("%-10s %5d keypoints, OK share %.3f, of those within 1 px of 20: %.3f" % (k, n, ok, good))
    assert shares["rectified"][0] >= 0.45
    assert shares["rectified"][0] >= 3.0 * shares["lens_only"][0]
    assert shares["rectified"][1] >= 0.99
    assert shares["raw"][0] < 0.2 and shares["lens_only"][0] < 0.2
    assert shares["ideal"][0] > shares["rectified"][0] and shares["ideal"][1] >= 0.99           # the control


def test_layout():
    import ctypes
    assert rr.lib().rr_params_size() == ctypes.sizeof(rr.Params) == 152
    assert rr.lib().rr_params_offset_R() == rr.Params.R.offset == 80 and rr.Params.lens.offset == 0
