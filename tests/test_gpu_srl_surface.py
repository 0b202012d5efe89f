"""ygz::StereoRelocalizer on the MI355X, through tests/cpp/srl_surface.cpp in a subprocess under a time limit.  The same small map is built
twice: three keyframes and three lost QVGA frames of a sequence whose pictures move by 3 pixels per frame (tests/stereo_ref.py's texture),
lattice keypoints that move with them, 70 % with the scene's constant depth, 90 % of a keyframe's features carrying the scene's point under
them; keyframe 2 shows an unrelated texture, and the third frame has 12 features only.  On one copy the host route runs frame by frame and
candidate by candidate: Matcher::SearchByBoW with checkOrientation off, the claim of ygz_reloc.cpp, ygz_hip_pnp_ransac, PoseOptimizer::Optimize
with PoseOptimizer::URightFromDepth from the PnP pose, the first candidate with at least 50 inliers wins; on the other ONE
StereoRelocalizer::Relocalize call runs with _check_orientation off.  _TCW (bitwise), the map point behind every feature, Feature::_bad,
Feature::_depth (bitwise) and _ref_keyframe must be equal, and no _cnt_found moves; the short frame, whose candidates all fail, is untouched;
no map point or keyframe appears; a single-frame call equals its batch entry."""
import os
import subprocess

import numpy as np
import pytest

import fixtures
import popt_ref
import stereo_ref as sr

pytestmark = pytest.mark.gpu
W, H, SHIFT, Z, NF, NK = 320, 240, 3, 4.0, 3, 3
K = popt_ref.DEFAULT_K
KF_AT = (0, 2, 0)                                                      # where in the sequence the keyframes stand; keyframe 2 on another texture
FRAME_AT = (1, 3, 2)
CANDS = ((2, 0, 1), (1, 0), (0, 1))
ENTRY = np.array([0, 0, 0, 1.0, 0.5, -0.25, 0.125])       # what a lost frame happens to hold


def pose(k):
    return np.array([0, 0, 0, 1.0, -k * SHIFT * Z / K[0], 0, 0])


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_srl_surface_build import build_program
    d = str(tmp_path_factory.mktemp("srl_gpu"))
    exe = build_program(d)
    rng = np.random.default_rng(47)
    src, other = sr.texture(W + 3 * SHIFT, H, 6), sr.texture(W + 3 * SHIFT, H, 60)
    px0, level = sr.lattice(W + 3 * SHIFT, H, 12)
    angle = rng.integers(0, 1440, len(level)) / 4.0
    P = len(level)
    # the map points: the lattice at the scene's depth, in the first camera's frame
    mp_pos = np.stack([(px0[:, 0] - K[2]) / K[0] * Z, (px0[:, 1] - K[3]) / K[1] * Z, np.full(P, Z)], 1)
    inside = lambda k: np.flatnonzero((px0[:, 0] - k * SHIFT >= 12) & (px0[:, 0] - k * SHIFT <= W - 12))
    with open(os.path.join(d, "vocab.bin"), "wb") as f:
        f.write(fixtures.synthetic_vocabulary(k=4, L=6, seed=11))
    mp_pos.tofile(os.path.join(d, "mp_pos.bin"))

    def write(tag, k, keep, entry, picture):
        np.ascontiguousarray(picture[:, k * SHIFT:k * SHIFT + W]).tofile(os.path.join(d, tag + "_img.bin"))
        np.stack([px0[keep, 0] - k * SHIFT, px0[keep, 1]], 1).astype(np.float64).tofile(os.path.join(d, tag + "_px.bin"))
        level[keep].astype(np.int32).tofile(os.path.join(d, tag + "_level.bin"))
        angle[keep].astype(np.float64).tofile(os.path.join(d, tag + "_angle.bin"))
        np.where(rng.uniform(size=len(keep)) < 0.7, Z, -1.0).tofile(os.path.join(d, tag + "_depth.bin"))
        entry.tofile(os.path.join(d, tag + "_pose.bin"))
    for j, k in enumerate(KF_AT):
        keep = inside(k)
        write("k%d" % j, k, keep, pose(k), other if j == 2 else src)
        np.where(rng.uniform(size=len(keep)) < 0.9, keep, -1).astype(np.int32).tofile(os.path.join(d, "k%d_mp.bin" % j))
    n = []
    for f, k in enumerate(FRAME_AT):
        keep = inside(k)
        if f == 2:
            keep = keep[:12]
        write("f%d" % f, k, keep, ENTRY, src)
        n.append(len(keep))
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return (lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype)), n, P


def results(ret, per):
    """(return value or None, winners [NF], per frame the rows of its candidates) of a _ret file with `per` numbers per candidate; the host
    route (per = 3) stops at a frame's winner"""
    ret = list(ret)
    first = ret.pop(0) if per == 4 else None
    win, rows = [], []
    for c in CANDS:
        win.append(ret.pop(0))
        m = win[-1] + 1 if per == 3 and win[-1] >= 0 else len(c)
        rows.append(np.array([ret.pop(0) for _ in range(m * per)], np.int64).reshape(m, per))
    assert not ret
    return first, win, rows


def test_one_call_equals_the_host_route(out):
    read, n, P = out
    assert read("batch_pose", np.float64).tobytes() == read("old_pose", np.float64).tobytes()
    for k in range(NF):
        for name, t in (("feat", np.int32), ("bad", np.uint8), ("depth", np.uint64)):
            a, b = read("old_%s%d" % (name, k), t), read("batch_%s%d" % (name, k), t)
            assert len(a) == n[k] and np.array_equal(a, b), (name, k)
    assert np.array_equal(read("old_ref", np.int32), read("batch_ref", np.int32)) and read("batch_ref", np.int32).tolist() == [0, 1, NK]
    assert np.array_equal(read("old_found", np.int32), read("batch_found", np.int32)) and (read("batch_found", np.int32) == 1).all()
    # the case is about something: the unrelated keyframe is passed over, the winners keep at least 50 features, the poses are the truth
    ret, win, rows = results(read("batch_ret", np.int32), 4)
    _, old_win, old_rows = results(read("old_ret", np.int32), 3)
    assert ret == 2 and win == old_win == [1, 0, -1]
    assert rows[0][:, 0].tolist() == [1, 0, 0] and rows[1][:, 0].tolist() == [0, 0] and rows[0][0, 1] < 15
    for f in range(NF):
        for q, o in enumerate(old_rows[f]):
            assert o[0] == rows[f][q, 1] and (o[1] < 0 or o[1] == rows[f][q, 2]) and (o[2] < 0 or o[2] == rows[f][q, 3]), (f, q)
    got = read("batch_pose", np.float64).reshape(NF, 7)
    assert np.abs(got[:2] - np.stack([pose(k) for k in FRAME_AT[:2]])).max() < 2e-3
    for f in range(2):
        feat = read("batch_feat%d" % f, np.int32)
        assert (feat >= 0).sum() == rows[f][win[f], 3] >= 50 and (feat >= -1).all()
        assert (read("batch_bad%d" % f, np.uint8)[feat >= 0] == 0).all()


def test_a_frame_whose_candidates_all_fail_is_untouched(out):
    read, n, _ = out
    _, win, rows = results(read("batch_ret", np.int32), 4)
    assert n[2] == 12 and win[2] == -1 and (rows[2][:, 0] == 1).all()
    assert (read("batch_feat2", np.int32) == -1).all() and not read("batch_bad2", np.uint8).any() and read("batch_ref", np.int32)[2] == NK
    assert read("batch_pose", np.float64).reshape(NF, 7)[2].tobytes() == ENTRY.tobytes()


def test_no_map_point_or_keyframe_appears(out):
    read = out[0]
    assert read("untouched", np.int32).tolist() == [1]


def test_single_frame_call_equals_its_batch_entry(out):
    read = out[0]
    one = read("single_ret", np.int32)
    _, win, rows = results(read("batch_ret", np.int32), 4)
    assert one[0] == 1 and one[1] == win[1] and np.array_equal(one[2:].reshape(-1, 4), rows[1])
    assert read("single_pose", np.float64).reshape(NF, 7)[1].tobytes() == read("batch_pose", np.float64).reshape(NF, 7)[1].tobytes()
    for name, t in (("feat", np.int32), ("bad", np.uint8), ("depth", np.uint64)):
        assert np.array_equal(read("single_%s1" % name, t), read("batch_%s1" % name, t)), name
    assert read("single_ref", np.int32)[1] == read("batch_ref", np.int32)[1]
