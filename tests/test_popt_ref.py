"""The restatement of the stereo pose optimisation (tests/popt_ref.c, the yardstick the device is held to bit for bit in tests/test_gpu_popt.py)
against a numpy witness of the same spec written another way, on the scenes of tests/popt_ref.py.  No device.

Measured (gcc 13, numpy 2, x86-64), and asserted at ten times that:
  - analytic Jacobian rows against the witness's central differences (step 1e-6 through the retraction), largest deviation relative to the
    edge's largest entry over every edge of every scene: 2.84e-10 -- bounded by the difference step, not by the code;
  - restatement against witness with the scenes' parameters: pose 7.50e-11 (absolute, unit quaternion and metres); cost_initial / cost_final
    4.14e-11 and chi2 8.86e-10 (relative, floor 1); lambda 7.25e-8 (relative: the cube of the gain ratio multiplies what the Jacobians differ
    by; an infinite lambda is infinite in both).  The two differ in the Jacobian, the summation order and the linear solve only.
Every discrete output -- outlier flags, inlier counts, rounds_run, round status, LM iteration counts and the accept / reject / fail / pivot
sequence of the trials -- is equal.  No edge of any scene is within 9 % of its threshold at the restatement's final pose (1 % is asked for).
  - with the library's defaults (min_rel_decrease = 0) the rounds run down to the rounding floor of the cost, where iteration counts and the
    trial sequence are decided by the last bit of a sum; what is stable there is held: flags, counts, rounds_run and which rounds FAILED equal,
    pose 7.32e-10 and chi2 1.51e-7 (scene b: mono edges alone leave the pose least determined), asserted at ten times that."""
import os
import subprocess

import numpy as np
import pytest

import popt_ref as pr

J_MEASURED, POSE_MEASURED, COST_MEASURED, CHI2_MEASURED, LAMBDA_MEASURED = 2.84e-10, 7.50e-11, 4.14e-11, 8.86e-10, 7.25e-8
POSE_DEFAULTS_MEASURED, CHI2_DEFAULTS_MEASURED = 7.32e-10, 1.51e-7


@pytest.fixture(scope="module")
def results():
    """name -> [(frame, parameters, restatement, witness)]: computed once, left unchanged"""
    out = {}
    for name in pr.SCENES:
        frames, p = pr.scene(name)
        out[name] = [(fr, p, pr.optimize(fr, p), pr.witness(fr, p)) for fr in frames]
    return out


def test_analytic_jacobian_against_central_differences():
    worst, seen = 0.0, {1: 0, 2: 0}
    for name in pr.SCENES:
        frames, p = pr.scene(name)
        for fr in frames:
            Jw = pr.w_jacobians(fr, fr.pose, pr.k5(p.baseline))
            for i in range(fr.n):
                kind = int(fr.kind[i])
                Ja = pr.jacobian(fr.pose, fr.X[i], kind) if kind else None
                if Ja is None:
                    continue
                rows = 3 if kind == 2 else 2
                assert not Ja[rows:].any()
                worst = max(worst, np.abs(Ja[:rows] - Jw[i, :rows]).max() / np.abs(Ja[:rows]).max())
                seen[kind] += 1
    print("largest relative deviation of a Jacobian: %.3g over %d mono and %d stereo edges" % (worst, seen[1], seen[2]))
    assert seen[1] > 1000 and seen[2] > 1000
    assert worst <= 10 * J_MEASURED, worst


def test_the_third_row_is_the_first_plus_the_disparity_term():
    fr = pr.scene("a")[0][0]
    for i in range(0, fr.n, 37):
        m, s = pr.jacobian(fr.pose, fr.X[i], 1), pr.jacobian(fr.pose, fr.X[i], 2)
        assert np.array_equal(m[:2], s[:2]) and np.array_equal(s[2, 2:4], s[0, 2:4]) and s[2, 4] == 0.0
        assert s[2, 5] != s[0, 5] and s[2, 0] != s[0, 0] and s[2, 1] != s[0, 1]


def rel(a, b):
    """largest deviation relative to max(|a|, 1); a value that is not finite has to be the same in both"""
    fin = np.isfinite(a)
    assert np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[~fin], b[~fin])
    return float((np.abs(a[fin] - b[fin]) / np.maximum(np.abs(a[fin]), 1.0)).max()) if fin.any() else 0.0


@pytest.mark.parametrize("name", pr.SCENES)
def test_restatement_equals_the_witness_at_the_defaults(name):
    worst = dict(pose=0.0, chi2=0.0)
    frames, p = pr.scene(name)
    p = pr.params(**dict(pr.fields(p), min_rel_decrease=0.0))
    for fr in frames:
        r, w = pr.optimize(fr, p), pr.witness(fr, p)
        assert np.array_equal(r["outlier"], w["outlier"]) and r["inliers"] == w["inliers"] and r["rounds_run"] == w["rounds_run"]
        assert np.array_equal(r["status"] == pr.FAILED, w["status"] == pr.FAILED)
        worst["pose"] = max(worst["pose"], float(np.abs(r["pose"] - w["pose"]).max()))
        worst["chi2"] = max(worst["chi2"], rel(r["chi2"], w["chi2"]))
    print("%s at the defaults: pose %.3g, chi2 %.3g" % (name, worst["pose"], worst["chi2"]))
    assert worst["pose"] <= 10 * POSE_DEFAULTS_MEASURED and worst["chi2"] <= 10 * CHI2_DEFAULTS_MEASURED, worst


@pytest.mark.parametrize("name", pr.SCENES)
def test_restatement_equals_the_witness(results, name):
    worst = dict(pose=0.0, cost=0.0, chi2=0.0, lam=0.0)
    for fr, p, r, w in results[name]:
        assert r["trace"] == w["trace"]
        assert np.array_equal(r["outlier"], w["outlier"]) and r["inliers"] == w["inliers"] and r["rounds_run"] == w["rounds_run"]
        assert np.array_equal(r["status"], w["status"]) and np.array_equal(r["lm_iterations"], w["lm_iterations"])
        assert r["inliers"] == int(((fr.kind != 0) & (r["outlier"] == 0)).sum())
        worst["pose"] = max(worst["pose"], float(np.abs(r["pose"] - w["pose"]).max()))
        worst["cost"] = max(worst["cost"], rel(r["cost_initial"], w["cost_initial"]), rel(r["cost_final"], w["cost_final"]))
        worst["chi2"] = max(worst["chi2"], rel(r["chi2"], w["chi2"]))
        worst["lam"] = max(worst["lam"], rel(r["lambda"], w["lambda"]))
        # unused rounds are zero
        k = r["rounds_run"]
        for key in pr.ROUND_OUTPUTS:
            assert not r[key][k:].any(), key
    print("%s: pose %.3g, cost %.3g, chi2 %.3g, lambda %.3g" % (name, worst["pose"], worst["cost"], worst["chi2"], worst["lam"]))
    assert worst["pose"] <= 10 * POSE_MEASURED and worst["cost"] <= 10 * COST_MEASURED, worst
    assert worst["chi2"] <= 10 * CHI2_MEASURED and worst["lam"] <= 10 * LAMBDA_MEASURED, worst


def test_no_edge_sits_near_its_threshold(results):
    smallest = np.inf
    for name in pr.SCENES:
        for fr, p, r, w in results[name]:
            th = np.where(fr.kind == 2, p.chi2_stereo, p.chi2_mono)
            m = (fr.kind != 0) & (r["chi2"] > 0)
            if m.any():
                smallest = min(smallest, float((np.abs(r["chi2"][m] - th[m]) / th[m]).min()))
    print("smallest margin of a chi2 to its threshold: %.3g" % smallest)
    assert smallest > 0.01


def test_the_scenes_reach_every_status_and_every_branch(results):
    one = lambda name: results[name][0]
    status, codes = set(), set()
    for name in pr.SCENES:
        for fr, p, r, w in results[name]:
            status |= set(int(s) for s in r["status"][:r["rounds_run"]])
            codes |= set(c for _, _, c in r["trace"])
    assert status == {pr.FAILED, pr.CONVERGED, pr.MAX_ITERATIONS, pr.STALLED}
    assert codes == {pr.TRIAL_ACCEPTED, pr.TRIAL_REJECTED, pr.TRIAL_FAILED, pr.TRIAL_PIVOT}
    # a, b, c: four CONVERGED rounds, all true inliers kept, all gross outliers found
    for name in ("a", "b", "c", "d", "i"):
        fr, p, r, w = one(name)
        assert r["rounds_run"] == 4 and (r["status"][:4] == pr.CONVERGED).all(), name
        assert np.array_equal(r["outlier"].astype(bool), fr.is_outlier), name
    # d: a later round changes flags
    fr, p, r, w = one("d")
    first = pr.optimize(fr, pr.params(rounds=1))
    assert (first["outlier"] != r["outlier"]).sum() >= 5
    # e: stops early on min_inliers
    fr, p, r, w = one("e")
    assert r["rounds_run"] < 4 and r["inliers"] < p.min_inliers and r["status"][0] != pr.FAILED
    # f, g: FAILED, the pose untouched bit for bit
    for name in ("f", "g"):
        fr, p, r, w = one(name)
        assert r["rounds_run"] == 1 and r["status"][0] == pr.FAILED and r["lm_iterations"][0] == 0 and r["pose"].tobytes() == fr.pose.tobytes(), name
        assert r["cost_initial"][0] == 0.0 and r["cost_final"][0] == 0.0 and r["lambda"][0] == 0.0
    assert one("g")[2]["outlier"].all() and not one("g")[2]["chi2"].any()          # rejected edges: outliers with chi2 0
    # h: kind 0 is never used and never classified; the results are those of the compacted list
    fr, p, r, w = one("h")
    c = pr.optimize(fr.compacted(), p)
    keep = fr.kind != 0
    assert (~keep).sum() == 100 and (r["chi2"][~keep] == -1.0).all() and not r["outlier"][~keep].any()
    assert r["inliers"] == c["inliers"] and np.array_equal(r["outlier"][keep], c["outlier"]) and r["trace"] == c["trace"]
    assert np.abs(r["pose"] - c["pose"]).max() < 1e-9                              # the lanes' shares differ: another summation order
    # j: every frame size; a single edge and three edges
    sizes = [fr.n for fr, p, r, w in results["j"]]
    assert tuple(sizes) == pr.J_SIZES
    assert results["j"][0][2]["status"][0] == pr.FAILED and results["j"][1][2]["status"][0] != pr.FAILED
    # k: the optimum of noise-free data: the step is zero, the gain is 0, the round is STALLED after one iteration and the pose keeps its bits
    fr, p, r, w = one("k")
    assert (r["status"][:4] == pr.STALLED).all() and (r["lm_iterations"][:4] == 1).all() and not r["cost_final"].any()
    assert r["trace"] == [(k, 0, pr.TRIAL_REJECTED) for k in range(4)] and r["pose"].tobytes() == fr.pose.tobytes()
    # l: the parameters
    assert one("l1r")[2]["rounds_run"] == 1 and (one("l1i")[2]["status"][:4] == pr.MAX_ITERATIONS).all()
    assert (one("l1i")[2]["lm_iterations"][:4] == 1).all()
    l0, l4, cc = one("l0")[2], one("l4")[2], one("c")[2]
    assert l0["cost_initial"][0] > cc["cost_initial"][0] and l4["cost_final"][3] != cc["cost_final"][3]      # no kernel in round 0; a kernel in round 3
    # m: one trial per iteration: STALLED by the trial count although the trial was accepted
    r = one("m")[2]
    assert (r["status"][:4] == pr.STALLED).all() and r["trace"] == [(k, 0, pr.TRIAL_ACCEPTED) for k in range(4)]
    # n: rejected trials are retried with a larger lambda inside one iteration, and trials fail on points behind the trial pose
    r = one("n")[2]
    its = [(k, it) for k, it, c in r["trace"]]
    assert len(its) > len(set(its)) and pr.TRIAL_FAILED in [c for _, _, c in r["trace"]] and r["inliers"] == 255
    # p: lambda_0 is infinite although the cost is finite: the pivot is not finite, lambda stays infinite, STALLED by the lambda rule
    r = one("p")[2]
    assert r["trace"] == [(0, 0, pr.TRIAL_PIVOT)] and r["status"][0] == pr.STALLED and r["cost_initial"][0] == 10.0 and np.isinf(r["lambda"][0])
    assert r["inliers"] == 5 and r["pose"].tobytes() == one("p")[0].pose.tobytes()
    # q: lambda grows through rejected trials until H + lambda I overflows; then the pivot fails with a finite lambda, trial after trial without
    # a pass (an infinite lambda ends the trials at once, so every pivot failure but the last had a finite one), until lambda itself overflows
    r = one("q")[2]
    codes = [c for _, _, c in r["trace"]]
    assert np.isinf(r["lambda"][0]) and np.isfinite(r["cost_initial"][0]) and r["status"][0] == pr.STALLED and len(codes) < 64
    assert codes[-4:] == [pr.TRIAL_PIVOT] * 4 and pr.TRIAL_REJECTED in codes and codes.count(pr.TRIAL_ACCEPTED) >= 2
    # r: H = 0 and lambda_0 = 0: every pivot fails, lambda stays 0, STALLED by the trial count
    r = one("r")[2]
    assert r["trace"] == [(0, 0, pr.TRIAL_PIVOT)] * 10 and r["status"][0] == pr.STALLED and r["lambda"][0] == 0.0 and r["lm_iterations"][0] == 1
    # o: edges rejected at the first linearisation are counted, not fatal: the rounds run and converge, the rejected edges end as outliers
    fr, p, r, w = one("o")
    L = pr.linearize(fr, fr.pose, p)
    assert L["n_rej"] == 18 and L["n_ok"] == 282 and r["rounds_run"] == 4 and (r["status"][:4] == pr.CONVERGED).all()
    assert r["outlier"][::17].all() and not r["chi2"][::17].any() and pr.TRIAL_FAILED not in [c for _, _, c in r["trace"]]


def test_scene_a_uses_the_third_residual(results):
    fr, p, r, w = results["a"][0]
    before, after = np.linalg.norm(fr.pose[4:] - fr.truth[4:]), np.linalg.norm(r["pose"][4:] - fr.truth[4:])
    print("translation error %.4f -> %.4f m" % (before, after))
    assert after < 0.2 * before
    mono = pr.optimize(fr.replace(kind=np.ones(fr.n, np.uint8)), p)
    assert np.abs(mono["pose"] - r["pose"]).max() > 1e-6 and mono["cost_final"][3] < r["cost_final"][3]
    # ... and it is the baseline that enters it
    wide = pr.optimize(fr, pr.params(baseline=0.2))
    assert np.abs(wide["pose"] - r["pose"]).max() > 1e-3


def test_the_summation_order():
    rng = np.random.RandomState(5)
    v = rng.randn(256) * 10.0 ** rng.randint(-8, 8, 256)
    wave = []
    for wv in range(4):
        rows = []
        for rw in range(4):
            x = list(v[64 * wv + 16 * rw:64 * wv + 16 * rw + 16])
            while len(x) > 1:
                x = [x[2 * i] + x[2 * i + 1] for i in range(len(x) // 2)]
            rows.append(x[0])
        wave.append(((rows[0] + rows[1]) + rows[2]) + rows[3])
    assert pr.reduce256(v) == ((wave[0] + wave[1]) + wave[2]) + wave[3]
    seq = 0.0
    for x in v:
        seq += x
    assert pr.reduce256(v) != seq                    # for these numbers the left-to-right sum is another double: an order, not just a sum


def test_linearisation_stage_against_the_witness():
    fr, p = pr.scene("c")[0][0], pr.scene("c")[1]
    for robust in (True, False):
        L = pr.linearize(fr, fr.pose, p, robust)
        d2 = np.where(fr.kind == 2, p.chi2_stereo, p.chi2_mono) if robust else np.zeros(fr.n)
        W = pr.w_pass(fr, fr.pose, pr.k5(p.baseline), fr.kind != 0, d2, True)
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = L["H"]
        H = H + np.triu(H, 1).T
        assert np.abs(H - W["H"]).max() <= 1e-8 * np.abs(H).max() and np.abs(L["b"] - W["b"]).max() <= 1e-8 * np.abs(L["b"]).max()
        assert abs(L["cost"] - W["cost"]) <= 1e-12 * L["cost"] and (L["n_ok"], L["n_rej"]) == (W["n_ok"], W["n_rej"]) == (300, 0)


def test_defaults_and_layout():
    p = pr.Params()
    pr.lib().pr_default_params(p)
    assert tuple(pr.fields(p).values()) == (0.0, 5.991, 7.815, 4, 10, 10, 3, 3, 10, 0.0)
    assert pr.lib().pr_params_size() == 56


def test_uright_from_depth_against_numpy(tmp_path):
    from test_popt_surface_build import build_program
    exe = build_program(str(tmp_path))
    rng = np.random.RandomState(3)
    n = 257
    px = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1)
    depth = rng.uniform(0.3, 40.0, n)
    depth[::7] = -1.0
    depth[3] = 0.0
    depth[5] = 0.01                                                   # uR far to the left of the picture: negative, so not a stereo edge
    px.tofile(os.path.join(str(tmp_path), "px.bin"))
    depth.tofile(os.path.join(str(tmp_path), "depth.bin"))
    r = subprocess.run([exe, "uright", str(tmp_path), "0.137"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(os.path.join(str(tmp_path), "u_right.bin"), np.float64)
    want = pr.uright_from_depth(px[:, 0], depth, 0.137)
    assert np.array_equal(got, want) and (got[::7] == -1.0).all() and got[3] == -1.0 and got[5] < -1.0
    count = np.fromfile(os.path.join(str(tmp_path), "count.bin"), np.int32)
    assert list(count) == [int((want >= 0).sum()), n]
