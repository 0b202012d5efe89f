"""tests/lms_ref.c, the restatement the device's local-map selection is held to, against a witness written another way: a dense K x P
incidence matrix, the votes of all frames as one masked matrix product, the extension as a Python loop over lists, the point set by `sorted`
over tuples and the prior through a dict.  The keyframe lists are also held to tests/strack_ref.py's local_keyframes, the plain-data form of
StereoTracker::LocalKeyFrames, on the same maps.  One hand-made case is compared against literal numbers, and the named cases against what
their construction forces."""
import numpy as np
import pytest

import lms_ref as lr
import strack_ref

CASES = lr.cases()
_ran = {}


def run(name):
    if name not in _ran:
        _ran[name] = lr.select(CASES[name])
    return _ran[name]


def witness(case):
    K, P, F = case["K"], len(case["off"]) - 1, len(case["fr_off"]) - 1
    q = dict(lr.DEFAULTS, **case["params"])
    inc = np.zeros((K, P), np.int32)
    feat = np.full((K, P), -1, np.int32)
    for p in range(P):
        s = slice(case["off"][p], case["off"][p + 1])
        inc[case["kf"][s], p] = 1
        feat[case["kf"][s], p] = case["feat"][s]
    good = np.ones(P, bool) if case["pt_bad"] is None else case["pt_bad"] == 0
    times = np.zeros((P, F), np.int32)                      # how often point p stands on frame f
    for f in range(F):
        pts = case["fr_pt"][case["fr_off"][f]:case["fr_off"][f + 1]]
        np.add.at(times[:, f], pts[pts >= 0], 1)
    votes = ((inc * good[None, :]) @ times).T               # [F][K]
    o = dict(votes=votes, ref=[], n_voters=[], n_local=[], local_kf=[], n_pt=[], n_cut=[], local_pt=[], fr_prior=[])
    for f in range(F):
        v = votes[f]
        o["ref"].append(int(np.argmax(v)) if v.max() > 0 else -1)           # argmax returns the first of equal maxima
        out = [int(k) for k in np.flatnonzero((v > 0) & (case["kf_bad"] == 0))]
        o["n_voters"].append(len(out))
        for k in list(out):
            if len(out) >= q["max_keyframes"]:
                break
            new = [int(c) for c in case["cov"][k] if c >= 0 and not case["kf_bad"][c] and c not in out]
            out += new[:1]
        o["n_local"].append(len(out))
        o["local_kf"].append(out + [-1] * (K - len(out)))
        keys = []
        if out:
            seen = inc[out] > 0                             # [rank][P]
            first = np.argmax(seen, axis=0)
            for p in np.flatnonzero(seen.any(axis=0) & good):
                keys.append((int(first[p]), int(feat[out[first[p]], p]), int(p)))
        pts = [p for _, _, p in sorted(keys)]
        kept = pts[:q["max_points"]]
        o["n_pt"].append(len(kept))
        o["n_cut"].append(len(pts) - len(kept))
        o["local_pt"].append(kept + [-1] * (q["max_points"] - len(kept)))
        where = {p: i for i, p in enumerate(kept)}
        o["fr_prior"] += [where.get(int(p), -1) for p in case["fr_pt"][case["fr_off"][f]:case["fr_off"][f + 1]]]
    return {k: np.asarray(v, np.int64).reshape(np.shape(lr.blank_outputs(case)[k]) if k != "fr_prior" else (-1,)) for k, v in o.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_c_equals_the_witness(name):
    got, ref = run(name), witness(CASES[name])
    for k in lr.OUTPUTS:
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("name", sorted(CASES))
def test_keyframe_lists_equal_the_tracker_rule(name):
    case, got = CASES[name], run(name)
    q = dict(lr.DEFAULTS, **case["params"])
    P = len(case["off"]) - 1
    points = {}
    for p in range(P):
        s = slice(case["off"][p], case["off"][p + 1])
        points[p] = dict(bad=bool(case["pt_bad"] is not None and case["pt_bad"][p]), obs=dict(zip(case["kf"][s].tolist(), case["feat"][s].tolist())))
    # a -1 of a row is looked at and skipped, and every entry of a row is looked at: the row without them, all of it
    keyframes = {k: dict(bad=bool(case["kf_bad"][k]), cov=[int(c) for c in case["cov"][k] if c >= 0]) for k in range(case["K"])}
    for f in range(len(case["fr_off"]) - 1):
        on_frame = [None if p < 0 else int(p) for p in case["fr_pt"][case["fr_off"][f]:case["fr_off"][f + 1]]]
        out, ref = strack_ref.local_keyframes(on_frame, points, keyframes, neighbours=lr.MAX_COV, max_keyframes=q["max_keyframes"])
        assert got["local_kf"][f, :got["n_local"][f]].tolist() == out and (got["local_kf"][f, got["n_local"][f]:] == -1).all(), f
        assert got["ref"][f] == (-1 if ref is None else ref), f


def test_hand_made_case_against_literal_numbers():
    got = run("hand")
    for k in lr.OUTPUTS:
        assert got[k].tolist() == lr.HAND_OUT[k], k


def test_the_named_cases_decide_what_they_were_built_for():
    g = run("frame_without_points")
    assert g["n_local"].tolist() == [0, 0, 4] and g["ref"].tolist() == [-1, -1, 1] and g["n_pt"].tolist()[:2] == [0, 0]
    assert (g["votes"][:2] == 0).all() and (g["local_kf"][:2] == -1).all() and g["fr_prior"].tolist()[:3] == [-1, -1, -1]
    g = run("point_twice")
    assert g["votes"][0].tolist() == [3, 2, 0, 1] and g["votes"][1].tolist() == [0, 1, 0, 3] and g["fr_prior"][0] == g["fr_prior"][2] >= 0
    g = run("bad_point_on_frame")
    assert g["votes"][0].tolist() == [1, 2, 0, 0] and g["votes"][1].tolist() == [0, 0, 0, 0] and g["fr_prior"].tolist()[1] == -1
    assert 3 not in g["local_pt"][0].tolist() and g["ref"].tolist() == [1, -1]
    g = run("bad_keyframe_most_votes")
    assert g["ref"].tolist() == [0] and g["votes"][0].tolist() == [2, 2, 0, 1] and g["local_kf"][0].tolist() == [1, 3, 2, -1]
    assert run("vote_tie")["ref"].tolist() == [1, 1]
    for n, (voters, local) in {5: (5, 6), 6: (6, 6), 7: (7, 7)}.items():
        g = run("voters%d_max6" % n)
        assert (g["n_voters"][0], g["n_local"][0]) == (voters, local), n
    assert run("voters5_max6")["local_kf"][0, 5] == 5 and run("voters3_max1")["n_local"].tolist() == [3]
    assert run("same_first_covisible")["local_kf"][0].tolist() == [0, 1, 2, 3, -1]
    assert run("covisible_row_of_none")["local_kf"][0].tolist() == [0, 1, 2]
    assert run("bad_first_covisible")["local_kf"][0].tolist() == [0, 3, -1, -1]
    assert run("covisible_is_a_voter")["local_kf"][0].tolist() == [0, 1, 2]
    g = run("no_covisibles")
    assert g["n_local"].tolist() == g["n_voters"].tolist() == [3, 1]
    g = run("point_of_two_local_keyframes")
    assert g["local_kf"][0, :2].tolist() == [1, 3] and g["local_pt"][0, :4].tolist() == [1, 0, 2, 3] and g["fr_prior"].tolist() == [0, 2]
    g = run("observers_outside_the_list")
    assert g["ref"].tolist() == [2] and g["local_kf"][0].tolist() == [0, 1, -1] and g["fr_prior"].tolist() == [-1, -1, 0]
    for mp, (n, cut) in {4: (4, 1), 5: (5, 0), 6: (5, 0)}.items():
        g = run("max_points%d_of5" % mp)
        assert (g["n_pt"][0], g["n_cut"][0]) == (n, cut) and g["local_pt"].shape == (2, mp), mp
    assert run("max_points4_of5")["fr_prior"].tolist() == [0, -1, 1, 0] and run("max_points1")["fr_prior"].tolist() == [0, -1, -1, 0]
    assert run("shared_feature")["local_pt"][0, :4].tolist() == [3, 1, 2, 0]
    for n in (63, 64, 65, 255, 256):
        case = CASES["list_of_%d" % n]
        assert case["off"][1] - case["off"][0] == n and run("list_of_%d" % n)["n_voters"][0] >= n
    for n in (255, 256, 257):
        assert (CASES["keyframe_of_%d" % n]["kf"] == 1).sum() >= n
    assert run("keyframe_of_256")["n_cut"][0] > 0
    assert run("k1_bad")["ref"].tolist() == [0, -1] and run("k1_bad")["n_local"].tolist() == [0, 0]
    g = run("k130_frames65")
    assert len(g["ref"]) == 65 and (g["n_cut"] > 0).any() and (g["n_cut"] == 0).any() and (g["n_local"] > g["n_voters"]).any()
    assert (run("k130_frames3")["n_local"] >= 20).all()
    g = run("k4096")
    assert CASES["k4096"]["K"] == 4096 and g["n_local"].max() > 2000 and (g["n_cut"] > 0).any()
