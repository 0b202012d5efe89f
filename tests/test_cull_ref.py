"""tests/cull_ref.c, the restatement the device's keyframe culling is held to, against a numpy witness written another way: a dense K x P
incidence matrix and a level matrix, the counts as masked sums, the walk as a Python loop that zeroes a column of the incidence (the removed
keyframe) and a row mask (the dead points).  One hand-made case is compared against literal numbers, and the named walks (ratio boundary,
order dependence, death cascade) against the decisions their construction forces."""
import numpy as np
import pytest

import cull_ref as cr

COUNTS = cr.count_cases()
WALKS = cr.walk_cases()


def _dense(case):
    K, P = case["K"], len(case["off"]) - 1
    inc, lev = np.zeros((P, K), bool), np.zeros((P, K), np.int64)
    for p in range(P):
        s = slice(case["off"][p], case["off"][p + 1])
        inc[p, case["kf"][s]] = True
        lev[p, case["kf"][s]] = case["level"][s]
    return inc, lev


def _witness_counts(inc, lev, alive, a, th_obs, level_slack):
    """alive [P]: the points that still count; inc has the removed keyframes' columns zeroed except a's own"""
    holds = inc[:, a] & alive
    others = inc.copy()
    others[:, a] = False
    if level_slack >= 0:
        others &= lev <= lev[:, [a]] + level_slack
    return int(holds.sum()), int((holds & (others.sum(axis=1) >= th_obs)).sum())


def witness_redundancy(case):
    q = dict(cr.DEFAULTS, **case["params"])
    inc, lev = _dense(case)
    if q["level_slack"] < 0:                  # every keyframe at once: the other observers of a point are its list less one
        many = inc.sum(axis=1) - 1 >= q["th_obs"]
        return dict(tracked=inc.sum(axis=0).astype(np.int32), redundant=(inc & many[:, None]).sum(axis=0).astype(np.int32))
    alive = np.ones(len(inc), bool)
    out = [_witness_counts(inc, lev, alive, a, q["th_obs"], q["level_slack"]) for a in range(case["K"])]
    return dict(tracked=np.array([t for t, _ in out], np.int32), redundant=np.array([r for _, r in out], np.int32))


def witness_walk(case):
    q = dict(cr.DEFAULTS, **case["params"])
    inc, lev = _dense(case)
    alive = np.ones(len(inc), bool)
    live = inc.sum(axis=1)
    o = dict(culled=[], tracked=[], redundant=[])
    for c in case["cand"]:
        t, r = _witness_counts(inc, lev, alive, c, q["th_obs"], q["level_slack"])
        hit = float(r) > q["ratio"] * float(t)
        o["culled"].append(int(hit)); o["tracked"].append(t); o["redundant"].append(r)
        if hit:
            live = live - inc[:, c]
            alive &= ~(inc[:, c] & (live < q["min_obs"]))
            inc[:, c] = False
    o = dict((k, np.array(v, np.int32)) for k, v in o.items())
    o["point_dead"] = (~alive).astype(np.uint8)
    return o


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_counts_equal_the_witness(name):
    case = COUNTS[name]
    got, ref = cr.run_counts(case), witness_redundancy(case)
    for k in ["tracked", "redundant"]:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("name", sorted(WALKS))
def test_walk_equals_the_witness(name):
    case = WALKS[name]
    got, ref = cr.run_walk(case), witness_walk(case)
    for k in ["culled", "tracked", "redundant", "point_dead"]:
        assert np.array_equal(got[k], ref[k]), k
    if name in cr.EXPECTED_CULLED:
        assert got["culled"].tolist() == cr.EXPECTED_CULLED[name]
    # the keyframe-major form of the same walk (the host baseline of tools/cull_bench.py)
    fast = cr.run_walk(case, lambda *a, **kw: cr.cull(*a, indexed=True, **kw))
    for k in ["culled", "tracked", "redundant", "point_dead"]:
        assert np.array_equal(fast[k], ref[k]), k


def test_hand_made_case_against_literal_numbers():
    got = cr.run_counts(COUNTS["hand_k5"])
    assert got["tracked"].tolist() == cr.HAND["tracked"] and got["redundant"].tolist() == cr.HAND["redundant"]
    for i, w in enumerate(cr.HAND["walks"]):
        got = cr.run_walk(WALKS["hand_k5_%d" % i])
        for k in ["culled", "tracked", "redundant", "point_dead"]:
            assert got[k].tolist() == w[k], (i, k)


def test_the_walk_with_one_candidate_is_the_counts_decision():
    for k in [3, 77, 129]:
        case = WALKS["one_kf%d" % k]
        walk, counts = cr.run_walk(case), cr.run_counts(case)
        assert walk["tracked"][0] == counts["tracked"][k] and walk["redundant"][0] == counts["redundant"][k]
        assert walk["culled"][0] == int(float(counts["redundant"][k]) > case["params"]["ratio"] * float(counts["tracked"][k]))


def test_the_cases_are_not_trivial():
    """every multi-candidate random walk culls some candidates and keeps some, and the big ones kill points"""
    for name in ["cand64", "cand65", "cand_all", "cand_all_ascending", "cand_all_levels", "subset", "big_first", "big_last", "column0"]:
        got = cr.run_walk(WALKS[name])
        assert 0 < got["culled"].sum() < len(got["culled"]), name
    assert cr.run_walk(WALKS["cand65"])["point_dead"].sum() > 0
    assert cr.run_walk(WALKS["cascade_ab_min2"])["point_dead"].tolist() == [0] * 20 + [1] + [0] * 9
    assert cr.run_walk(WALKS["cascade_ab_min0"])["point_dead"].sum() == 0
