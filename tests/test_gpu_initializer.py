"""The monocular Initializer on the MI355X (ygz_hip_initialize and its stages, ygz_slam_amd/csrc/init.hip) against the restatement of
src/Algorithm/Initializer.cpp in tests/init_ref.c: sample sets, all 200 H and F models and scores, the model choice, the reconstruction
and the triangulated points bit for bit (the parallax, which goes through acos, to 1e-12 relative), the fused call equal to its stages
chained, the recovered motion of the general scenes within bounds of the ground truth, degenerate inputs refused or failed without a
fault, and the class surface (ygz::Initializer in libygz_host.so) equal to the ABI call."""
import os
import subprocess

import numpy as np
import pytest

import init_ref as ir
from conftest import ROOT

pytestmark = pytest.mark.gpu

# (name, n, planar, outliers, seed)
SCENES = [("general50", 50, False, 0.0, 11), ("general50_out", 50, False, 0.1, 12), ("general600", 600, False, 0.0, 13),
          ("general600_out", 600, False, 0.1, 14), ("general3072", 3072, False, 0.0, 15), ("general3072_out", 3072, False, 0.1, 16),
          ("planar400", 400, True, 0.0, 17)]
# bounds of the recovered motion on the general scenes (rotation error, angle between t21 and the true direction, degrees): the restatement's
# own run on these scenes stays below 0.6 / 5.2 (init_ref.c, noise 0.5 px); the bounds leave about twice that
ROT_BOUND_DEG, T_BOUND_DEG = 1.5, 10.0
REC_FIELDS = ["success", "model", "n_inliers", "solution", "n_good", "second_good", "similar", "n_triangulated"]   # what a reconstruction reports


def _eq(a, b):
    """bit-equal arrays; NaN (a hypothesis whose sample is degenerate) equals NaN -- the device and the host CPU spell NaN differently"""
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b)


def _scene(name):
    if name in ("refH", "refF"):
        g = np.load(os.path.join(ROOT, "tests", "golden", "init_reference_scenes.npz"))
        P = g["landmarks_H" if name == "refH" else "landmarks_F"]
        K4 = g["K4"]
        return dict(px1=ir.project(K4, P), px2=ir.project(K4, P + g["t2"]), K4=K4, R=np.eye(3), t=g["t2"])
    _, n, planar, out, seed = [s for s in SCENES if s[0] == name][0]
    return ir.scene(n, seed, planar=planar, outliers=out)


ALL = [s[0] for s in SCENES] + ["refH", "refF"]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


def _same_result(a, b, parallax=True):
    for k in REC_FIELDS:
        assert a[k] == b[k], (k, a[k], b[k])
    for k in ["R21", "t21", "T21"]:
        assert _eq(a[k], b[k]), (k, a[k], b[k])
    if parallax:
        assert a["parallax"] == b["parallax"] or abs(a["parallax"] - b["parallax"]) <= 1e-12 * abs(b["parallax"]), (a["parallax"], b["parallax"])


@pytest.mark.parametrize("name", ALL)
def test_sample_sets_equal_the_restatement(hip_lib, name):
    n = len(_scene(name)["px1"])
    s = hip_lib.init_sample_sets(n, 200)
    assert _eq(s, ir.sample_sets(n, 200))


@pytest.mark.parametrize("name", ALL)
def test_hypotheses_bit_identical(ctx, name):
    s = _scene(name)
    g = ctx.init_hypotheses(s["px1"], s["px2"])
    r = ir.hypotheses(s["px1"], s["px2"], ir.sample_sets(len(s["px1"]), 200))
    assert _eq(g["H21"], r["H21"]) and _eq(g["F21"], r["F21"])
    assert _eq(g["score_h"], r["score_h"]) and _eq(g["score_f"], r["score_f"])
    assert _eq(g["inliers_h"], r["inliers_h"]) and _eq(g["inliers_f"], r["inliers_f"])
    for k in ["best_h", "best_f", "model"]:
        assert g["result"][k] == r["result"][k], k
    for k in ["score_h", "score_f", "rh"]:
        assert _eq(np.float32(g["result"][k]), np.float32(r["result"][k])), k
    assert _eq(g["result"]["H21"], r["result"]["H21"]) and _eq(g["result"]["F21"], r["result"]["F21"])


@pytest.mark.parametrize("name", ALL)
def test_fused_call_bit_identical_to_the_restatement(ctx, name):
    s = _scene(name)
    g = ctx.initialize(s["px1"], s["px2"], s["K4"])
    r = ir.initialize(s["px1"], s["px2"], s["K4"])
    _same_result(g, r["result"])
    for k in ["best_h", "best_f"]:
        assert g[k] == r["result"][k], k
    assert _eq(g["H21"], r["result"]["H21"]) and _eq(g["F21"], r["result"]["F21"])
    assert _eq(g["pts3d"], r["pts3d"]) and _eq(g["triangulated"], r["triangulated"])
    # no decision of the fixture sits within the parallax tolerance of its threshold
    if g["solution"] >= 0:
        assert abs(g["parallax"] - 1.0) > 1e-9


@pytest.mark.parametrize("name", ALL)
def test_fused_call_equals_the_stages_chained(ctx, name, hip_lib):
    s = _scene(name)
    g = ctx.initialize(s["px1"], s["px2"], s["K4"])
    h = ctx.init_hypotheses(s["px1"], s["px2"])
    m = h["result"]["model"]
    assert g["model"] == m and g["best_h"] == h["result"]["best_h"] and g["best_f"] == h["result"]["best_f"]
    if m == hip_lib.INIT_NONE:
        assert not g["success"]
        return
    M = h["result"]["H21"] if m == hip_lib.INIT_H else h["result"]["F21"]
    inl = h["inliers_h"] if m == hip_lib.INIT_H else h["inliers_f"]
    c = ctx.init_reconstruct(s["px1"], s["px2"], s["K4"], m, M, inl)
    _same_result(g, c, parallax=False)
    assert g["parallax"] == c["parallax"]
    assert _eq(g["pts3d"], c["pts3d"]) and _eq(g["triangulated"], c["triangulated"])


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("model", [1, 2])
def test_reconstruct_from_either_model_bit_identical(ctx, name, model):
    """ReconstructH is covered here even where the fused path chooses F (rh ~ 1/3 when F fits: DESIGN.md section 9)"""
    s = _scene(name)
    h = ir.hypotheses(s["px1"], s["px2"], ir.sample_sets(len(s["px1"]), 200))
    assert (h["result"]["best_h"] if model == 1 else h["result"]["best_f"]) >= 0
    M = h["result"]["H21"] if model == 1 else h["result"]["F21"]
    inl = h["inliers_h"] if model == 1 else h["inliers_f"]
    g = ctx.init_reconstruct(s["px1"], s["px2"], s["K4"], model, M, inl)
    r = ir.reconstruct(s["px1"], s["px2"], s["K4"], model, M, inl)
    _same_result(g, r["result"])
    assert _eq(g["pts3d"], r["pts3d"]) and _eq(g["triangulated"], r["triangulated"])


@pytest.mark.parametrize("name", [s[0] for s in SCENES if not s[2]])
def test_general_scene_motion_within_bounds(ctx, name):
    s = _scene(name)
    g = ctx.initialize(s["px1"], s["px2"], s["K4"])
    assert g["success"] and g["model"] == 2
    R = g["R21"].reshape(3, 3)
    rot = np.degrees(np.arccos(np.clip((np.trace(R.T @ s["R"]) - 1) / 2, -1, 1)))
    tdir = np.degrees(np.arccos(np.clip(g["t21"] @ s["t"] / np.linalg.norm(s["t"]), -1, 1)))
    assert rot < ROT_BOUND_DEG and tdir < T_BOUND_DEG, (rot, tdir)
    assert g["n_triangulated"] >= 0.8 * len(s["px1"]) * (0.9 if "out" in name else 1.0)


def test_reference_scenes(ctx):
    """test/test_initializer.cpp's scenes without its cv::RNG noise: the planar one fails (F is chosen at rh = 1/3 and no solution has
    0.9 of the inliers), the three-plane one succeeds with R21 = I and t21 along (1, 0, 0)"""
    g = ctx.initialize(**{k: v for k, v in _scene("refH").items() if k in ("px1", "px2", "K4")})
    assert not g["success"] and g["model"] == 2
    g = ctx.initialize(**{k: v for k, v in _scene("refF").items() if k in ("px1", "px2", "K4")})
    assert g["success"]
    assert np.abs(g["R21"].reshape(3, 3) - np.eye(3)).max() < 1e-9
    assert np.abs(g["t21"] - np.array([1.0, 0, 0])).max() < 1e-9


def test_degenerate_inputs(ctx, hip_lib):
    K4 = ir.K4_DEFAULT
    s = ir.scene(200, 21)
    # zero motion: no solution is accepted
    g = ctx.initialize(s["px1"], s["px1"], K4)
    r = ir.initialize(s["px1"], s["px1"], K4)
    assert not g["success"]
    _same_result(g, r["result"])
    # every point identical: nothing scores, no model
    same = np.tile([[320.0, 240.0]], (100, 1))
    g = ctx.initialize(same, same, K4)
    assert not g["success"] and g["model"] == hip_lib.INIT_NONE and g["best_h"] == -1 and g["best_f"] == -1
    _same_result(g, ir.initialize(same, same, K4)["result"])
    # exactly eight points
    e = ir.scene(8, 22)
    g = ctx.initialize(e["px1"], e["px2"], K4)
    _same_result(g, ir.initialize(e["px1"], e["px2"], K4)["result"])
    assert _eq(g["pts3d"], ir.initialize(e["px1"], e["px2"], K4)["pts3d"])
    # refused before anything is launched
    for n in (0, 7):
        with pytest.raises(hip_lib.YgzHipError) as ei:
            ctx.initialize(s["px1"][:n], s["px2"][:n], K4)
        assert ei.value.code == hip_lib.E_INVALID
    big = ir.scene(ctx.cells + 1, 23)
    with pytest.raises(hip_lib.YgzHipError) as ei:
        ctx.initialize(big["px1"], big["px2"], K4)
    assert ei.value.code == hip_lib.E_CAPACITY
    with pytest.raises(hip_lib.YgzHipError) as ei:
        ctx.initialize(s["px1"], s["px2"], K4, max_iter=0)
    assert ei.value.code == hip_lib.E_INVALID
    # the context still works afterwards
    g = ctx.initialize(s["px1"], s["px2"], K4)
    assert g["success"]


def test_class_surface_equals_the_abi_call(ctx, tmp_path):
    """ygz::Initializer::TryInitialize / GetT21 / GetTriangluatedPoints (tests/cpp/init_surface.cpp, built by test_init_surface_build's
    recipe) on the device: the same T21 and points as ygz_hip_initialize"""
    from test_init_surface_build import build_program
    exe = build_program(str(tmp_path))
    s = ir.scene(600, 13)
    inp = tmp_path / "in.txt"
    with open(inp, "w") as f:
        f.write("%d\n" % len(s["px1"]))
        for a, b in zip(s["px1"], s["px2"]):
            f.write("%.17g %.17g %.17g %.17g\n" % (a[0], a[1], b[0], b[1]))
    out = subprocess.check_output([exe, str(inp)], timeout=120, env=dict(os.environ, YGZ_HIP_DEVICE="0")).decode().split("\n")
    head = out[0].split()
    assert head[0] == "ok" and int(head[1]) == 1
    T = np.array([float(v) for v in out[1].split()])
    pts = np.array([[float(v) for v in ln.split()] for ln in out[2:2 + len(s["px1"])]])
    g = ctx.initialize(s["px1"], s["px2"], ir.K4_CONFIG)
    assert _eq(T, g["T21"])
    tri = pts[:, 3].astype(bool)
    assert _eq(tri, g["triangulated"])
    assert _eq(pts[tri, :3], g["pts3d"][tri])
