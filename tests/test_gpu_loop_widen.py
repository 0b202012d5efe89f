"""ygz::LoopClosing::SearchLoopMapPoints and Matcher::SearchBySim3 / SearchByProjection / SearchFuseCandidates on the MI355X, on the rendered
loop scene of tests/test_gpu_loop_closing.py (an old keyframe map, a revisit run in a world drifted by s = 1.2, 4 degrees, 10 cm): after the
ComputeSim3 that accepts the loop, SearchLoopMapPoints returns true with at least 40 matches and more than the refined inliers, no keypoint
and no loop point is matched twice, the map is unchanged, each Matcher method equals tests/proj_ref.c on the arrays the program gathered by
the documented rules, and every match lies where the current keyframe's TRUE pose puts its loop point, within the search radius plus the
pixel effect of the scene's bounds on the Sim3.  The program runs in a subprocess under a time limit (tests/widen_driver.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import proj_ref as pr

pytestmark = pytest.mark.gpu

W, H, L = 640, 480, 3
# the loop scene's bounds on the accepted Sim3 (tests/test_gpu_loop_closing.py): scale 1 %, rotation 0.25 degrees, translation 1 cm
S_BOUND, R_BOUND_DEG, T_BOUND_M = 0.01, 0.25, 0.01
KEYS = ("kp_px", "kp_level", "kp_desc", "kp_taken", "pw", "pt_desc", "pt_dmax", "pt_normal", "pt_skip", "S")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from test_proj_surface_build import build_program
    d = tmp_path_factory.mktemp("widen_gpu")
    so = build_program(str(d))
    out = os.path.join(str(d), "widen.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "widen_driver.py"), so, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = dict(np.load(out))
    o = z["out"]
    print("loop at revisit keyframe %d with keyframe %d: %d refined inliers, SearchBySim3 +%d, %d loop points, SearchByProjection +%d, total %d; "
          "fuse over %d keyframes: %d hits" % (o[1], o[2], o[3], o[5], o[15], o[6], o[7], o[16], o[13]))
    assert o[0] == 1, "no loop was accepted"
    return z


def _problem(z, prefix):
    d = {k: z[prefix + k] for k in KEYS if prefix + k in z}
    d["kp_px"] = d["kp_px"].reshape(-1, 2); d["kp_desc"] = d["kp_desc"].reshape(-1, 32)
    d["pw"] = d["pw"].reshape(-1, 3); d["pt_desc"] = d["pt_desc"].reshape(-1, 32)
    if "pt_normal" in d:
        d["pt_normal"] = d["pt_normal"].reshape(-1, 3)
    return d


def test_search_loop_map_points_accepts_the_loop(run):
    o = run["out"]
    assert o[4] == 1
    assert o[7] >= 40 and o[7] > o[3], o[:8]
    assert o[5] >= 0 and o[6] > 0, o[:8]
    assert o[7] == o[3] + o[5] + o[6], o[:8]
    assert o[17] == 1                                     # a second call gives the same vector


def test_nothing_is_matched_twice(run):
    fin = run["final"]
    hit = fin[fin != -1]
    assert (hit >= 0).all()                               # every matched point is a loop map point
    assert len(hit) == run["out"][7] and len(set(hit.tolist())) == len(hit)
    # a keypoint holds one point by construction; no search wrote over an earlier one
    s3, sp = run["s3_result"], run["sp_result"]
    assert not ((sp >= 0) & (s3 != -1)).any()
    added = s3[s3 >= 0]
    assert len(set(added.tolist())) == len(added)


def test_map_is_unchanged_and_the_class_equals_its_steps(run):
    o = run["out"]
    assert o[8] == 1 and o[9] == 1 and o[10] == 1
    assert o[5] == o[11] and o[6] == o[12]


def test_search_by_sim3_equals_the_restatement(run):
    a, b = _problem(run, "s3a_"), _problem(run, "s3b_")
    assert "pt_normal" not in a and a["S"][7] != 1.0 and b["S"][7] != 1.0            # no viewing-angle test, the scale is kept
    n1 = len(a["pt_dmax"])
    m = pr.search([a, b], K4=run["K4"], w=W, h=H, L=L, th=7.5, th_dist=100, claim=0)["match"]
    ma, mb = m[:n1], m[n1:]
    exp = np.array([ma[i] if ma[i] >= 0 and mb[ma[i]] == i else -1 for i in range(n1)])
    got = run["s3_result"]
    seeds = got == -2
    assert seeds.sum() == run["out"][3] and (a["pt_skip"][seeds] == 1).all()
    assert np.array_equal(got[~seeds], exp[~seeds]) and (exp[seeds] == -1).all()
    assert (got >= 0).sum() == run["out"][11]


def test_search_by_projection_equals_the_restatement(run):
    p = _problem(run, "sp_")
    assert p["S"][7] == 1.0 and "pt_normal" in p
    ref = pr.search([p], K4=run["K4"], w=W, h=H, L=L, th=10.0, th_dist=50, claim=1)
    exp = np.full(len(p["kp_level"]), -1)
    for i, j in enumerate(ref["match"]):
        if j >= 0:
            exp[j] = i
    assert np.array_equal(run["sp_result"], exp)
    assert ref["counts"][0, 0] == run["out"][12] > 0


def test_fuse_candidates_equal_the_restatement(run):
    K = int(run["out"][16])
    got = run["fu_result"].reshape(K, -1)
    assert K >= 2 and got.shape[1] == run["out"][15]
    ps = [_problem(run, "fu%d_" % k) for k in range(K)]
    ref = pr.search(ps, K4=run["K4"], w=W, h=H, L=L, th=3.0, th_dist=50, claim=0)
    assert np.array_equal(got.reshape(-1), ref["match"])
    assert (got >= 0).sum() == run["out"][13] > 0
    for k in range(K):                                     # a keyframe's own points are skipped
        assert ps[k]["pt_skip"].sum() > 0 and (got[k][ps[k]["pt_skip"] == 1] == -1).all()


def _R(q):
    x, y, z, w = np.asarray(q) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_every_match_agrees_with_the_true_pose(run):
    """The old world is the true world, so the current keyframe's true pose T1 projects a loop point to where its keypoint must be: within the
    window the search used (th 2^pred round the ESTIMATED projection) plus what the Sim3's error moves the projection by.  With the scene's
    bounds (scale e, rotation a, translation dt on S_cw = (s R1, s t1)) the search's camera point R P + t / s differs from the true R1 P + t1
    by a rotation of at most a, which moves a ray at off-axis tangent rho by f (tan(atan(rho) + a) - rho) pixels, and by a translation of at
    most b = (dt + e |s t1|) / (s (1 - e)), which moves a point at depth z >= zmin by at most f b (1 + rho) / (zmin - b) pixels; rho at the
    image corner, f the larger focal length."""
    K4, T1 = run["K4"], run["rev_T"][int(run["out"][1])]
    s_d, zmin = run["drift"][7], float(run["zmin"])
    f = max(K4[0], K4[1])
    rho = np.hypot(max(K4[2], W - K4[2]) / K4[0], max(K4[3], H - K4[3]) / K4[1])
    a = np.deg2rad(R_BOUND_DEG)
    b = (T_BOUND_M + S_BOUND * s_d * np.linalg.norm(T1[4:])) / (s_d * (1 - S_BOUND))
    allowance = f * (np.tan(np.arctan(rho) + a) - rho) + f * b * (1 + rho) / (zmin - b)
    print("allowance %.2f px (zmin %.3f m)" % (allowance, zmin))
    assert 0 < allowance < 10
    P = run["loop_pw"].reshape(-1, 3)
    Xc = P @ _R(T1[:4]).T + T1[4:]
    uv = np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], 1)
    px = run["cur_px"].reshape(-1, 2)
    # SearchByProjection's matches: radius 10 2^pred with the restatement's predicted level of that loop point
    pred = pr.candidates(_problem(run, "sp_"), K4=K4, w=W, h=H, L=L, th=10.0, th_dist=50)["pred_level"]
    sp = run["sp_result"]
    worst = 0.0
    for j in np.nonzero(sp >= 0)[0]:
        i = sp[j]
        assert pred[i] >= 0
        err = np.abs(uv[i] - px[j]).max()
        worst = max(worst, err - 10.0 * 2 ** pred[i])
        assert err < 10.0 * 2 ** pred[i] + allowance, (j, i, err, pred[i])
    # SearchBySim3's pairs: the loop keyframe's point into the current keyframe, radius 7.5 2^pred
    predb = pr.candidates(_problem(run, "s3b_"), K4=K4, w=W, h=H, L=L, th=7.5, th_dist=100)["pred_level"]
    s3, lfp = run["s3_result"], run["loop_feature_point"]
    for j in np.nonzero(s3 >= 0)[0]:
        j2 = s3[j]
        i = lfp[j2]
        assert i >= 0 and predb[j2] >= 0 and run["final"][j] == i
        err = np.abs(uv[i] - px[j]).max()
        assert err < 7.5 * 2 ** predb[j2] + allowance, (j, j2, err, predb[j2])
    print("largest excess over the radius: %.2f px" % worst)
