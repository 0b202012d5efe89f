"""ygz::PoseOptimizer on the MI355X: Optimize on frames built from scenes c and a of tests/popt_ref.py equals the C call on the gathered arrays
-- which is the restatement -- and leaves on the frame what ba::OptimizeCurrentPoseOnly leaves: _TCW, Feature::_bad for the outliers, _depth
and the map point's _cnt_found for the inliers, nothing on a feature that was no edge; OptimizeBatch equals the single calls; URightFromDepth
followed by Optimize turns depth features into stereo edges.  The program tests/cpp/popt_surface.cpp runs in a subprocess under a time limit."""
import os
import subprocess

import numpy as np
import pytest

import popt_ref as pr

pytestmark = pytest.mark.gpu
EXTRA = 4                 # features of frame 0 that are no edges


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    from test_popt_surface_build import build_program
    d = str(tmp_path_factory.mktemp("popt_gpu"))
    exe = build_program(d)
    frames = [pr.scene("c")[0][0], pr.scene("a")[0][0]]
    for q, fr in enumerate(frames):
        for name in ("pose", "obs", "level", "kind"):
            getattr(fr, name).tofile(os.path.join(d, "f%d_%s.bin" % (q, name)))
        fr.X.tofile(os.path.join(d, "f%d_pw.bin" % q))
    r = subprocess.run([exe, "run", d], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return frames, (lambda name, dtype: np.fromfile(os.path.join(d, name + ".bin"), dtype))


def test_optimize_equals_the_c_call_and_the_restatement(out):
    frames, f = out
    for q, fr in enumerate(frames):
        want = pr.optimize(fr, pr.defaults())
        s, a = "s%d_" % q, "abi%d_" % q
        assert f(a + "pose", np.float64).tobytes() == want["pose"].tobytes() == f(s + "pose", np.float64).tobytes()
        assert np.array_equal(f(a + "outlier", np.uint8), want["outlier"])
        assert list(f(a + "counts", np.int32)) == [want["inliers"], want["rounds_run"]] and np.array_equal(f(a + "status", np.int32), want["status"])
        ret = f(s + "ret", np.int32)
        assert list(ret) == [want["inliers"], want["inliers"], want["rounds_run"]]
        assert np.array_equal(f(s + "status", np.int32), want["status"][:want["rounds_run"]])
        assert np.array_equal(f(s + "outlier", np.uint8)[:fr.n], want["outlier"])


def test_the_frame_is_left_as_optimize_current_pose_only_leaves_it(out):
    frames, f = out
    for q, fr in enumerate(frames):
        want = pr.optimize(fr, pr.defaults())
        s = "s%d_" % q
        extra = EXTRA if q == 0 else 0
        bad, depth, found, flags = f(s + "bad", np.uint8), f(s + "depth", np.float64), f(s + "found", np.int32), f(s + "outlier", np.uint8)
        assert len(bad) == len(depth) == len(found) == len(flags) == fr.n + extra
        outl = want["outlier"].astype(bool)
        assert np.array_equal(bad[:fr.n].astype(bool), outl)
        z = (pr.w_rotation(want["pose"]) @ fr.X.T).T[:, 2] + want["pose"][6]
        assert np.abs(depth[:fr.n][~outl] - z[~outl]).max() < 1e-12 and (depth[:fr.n][outl] == -1.0).all()     # the outliers keep their depth
        assert (found[:fr.n][~outl] == 1).all() and (found[:fr.n][outl] == 0).all()
        if extra:                                                   # no map point, or a bad one: no edge, nothing touched
            assert not bad[fr.n:].any() and (depth[fr.n:] == -1.0).all() and not flags[fr.n:].any() and list(found[fr.n:]) == [-1, -1, -1, 0]
    assert (f("s0_bad", np.uint8) != 0).sum() == frames[0].is_outlier.sum() == 45


def test_batch_equals_the_single_calls(out):
    frames, f = out
    poses = f("b_pose", np.float64).reshape(2, 7)
    assert poses[0].tobytes() == f("s0_pose", np.float64).tobytes() and poses[1].tobytes() == f("s1_pose", np.float64).tobytes()
    assert np.array_equal(f("b_bad", np.uint8), np.concatenate([f("s0_bad", np.uint8), f("s1_bad", np.uint8)]))
    assert list(f("b_inliers", np.int32)) == [f("s0_ret", np.int32)[0], f("s1_ret", np.int32)[0]]


def test_uright_from_depth_makes_stereo_edges(out):
    frames, f = out
    fr = frames[0]
    cnt, stereo = f("d_count", np.int32)
    assert stereo == int((fr.kind == 2).sum()) == 150
    # the program gives every stereo edge the depth bf / (u - uR); where noise or a gross displacement made the disparity negative there is no
    # depth, and the feature is a mono edge.  u -> depth -> u_right costs two roundings, stated here in numpy
    bf = pr.DEFAULT_K[0] * 0.1
    disp = fr.obs[:, 0] - fr.obs[:, 2]
    assert disp.all()
    depth = np.where(fr.kind == 2, bf / disp, -1.0)
    ur = pr.uright_from_depth(fr.obs[:, 0], depth, 0.1)
    back = ur >= 0
    assert cnt == int(back.sum()) and 100 < cnt < 150
    obs = fr.obs.copy()
    obs[back, 2] = ur[back]
    want = pr.optimize(fr.replace(obs=obs, kind=np.where(back, 2, 1).astype(np.uint8)), pr.defaults())
    d, s, m = f("d_pose", np.float64), f("s0_pose", np.float64), f("m_pose", np.float64)
    assert d.tobytes() == want["pose"].tobytes() and f("d_ret", np.int32)[0] == want["inliers"]
    assert np.abs(d - s).max() < np.abs(m - s).max() and np.abs(m - d).max() > 1e-5       # nearer the stereo result than the mono one is
    mono = pr.optimize(fr.replace(kind=np.ones(fr.n, np.uint8)), pr.defaults())
    assert m.tobytes() == mono["pose"].tobytes()
