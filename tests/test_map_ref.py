"""tests/map_ref.c, the restatement the map-upkeep calls are held to (tests/test_gpu_map.py), against numpy witnesses written another way, on
the same small cases: np.sort of each distance row and np.argmin for the distinctive descriptors, A.T @ A of the point x keyframe incidence
matrix for the covisibility weights."""
import numpy as np
import pytest

import map_ref as mr

DESC = mr.descriptor_cases()
WEIGHTS = mr.weight_cases()


def _witness_distinctive(off, desc):
    P = len(off) - 1
    best, med, out = np.full(P, -1, np.int32), np.full(P, -1, np.int32), np.zeros((P, 32), np.uint8)
    bits = np.unpackbits(desc.reshape(-1, 32), axis=1).astype(np.int32)
    for p in range(P):
        a, b = off[p], off[p + 1]
        n = b - a
        if n == 0:
            continue
        x = bits[a:b]
        d = (x[:, None, :] != x[None, :, :]).sum(axis=2)
        m = np.sort(d, axis=1)[:, (n - 1) // 2]
        best[p] = int(np.argmin(m))                                  # the first of the smallest
        med[p] = m[best[p]]
        out[p] = desc[a + best[p]]
    return best, med, out


@pytest.mark.parametrize("name", sorted(DESC))
def test_distinctive_restatement_equals_sorted_rows(name):
    off, desc = DESC[name]
    r = mr.distinctive(off, desc)
    best, med, out = _witness_distinctive(off, desc)
    assert np.array_equal(r["best"], best) and np.array_equal(r["median"], med) and np.array_equal(r["desc"], out)


def test_distinctive_cases_hold_what_they_are_for():
    r = mr.distinctive(*DESC["identical"])
    assert list(r["best"]) == [0, 0] and list(r["median"]) == [0, 0]
    r = mr.distinctive(*DESC["n0"])
    assert list(r["best"]) == [-1] and list(r["median"]) == [-1] and not r["desc"].any()
    # the clustered cases tie: some point has two observations with the smallest median
    tied = 0
    for name in ["clustered", "clustered_tight", "batch300"]:
        off, desc = DESC[name]
        bits = np.unpackbits(desc, axis=1).astype(np.int32)
        for p in range(len(off) - 1):
            x = bits[off[p]:off[p + 1]]
            m = np.sort((x[:, None, :] != x[None, :, :]).sum(axis=2), axis=1)[:, (len(x) - 1) // 2]
            tied += int((m == m.min()).sum() > 1)
    assert tied >= 5
    counts = np.diff(DESC["batch300"][0])
    assert len(counts) == 300 and counts.min() >= 1 and counts.max() <= 12 and counts.sum() > 1024


@pytest.mark.parametrize("name", sorted(WEIGHTS))
def test_covisibility_restatement_equals_incidence_product(name):
    off, kf, K, rows = WEIGHTS[name]
    P = len(off) - 1
    A = np.zeros((P, K), np.int64)
    for p in range(P):
        A[p, kf[off[p]:off[p + 1]]] = 1
    full = A.T @ A
    assert np.array_equal(mr.covisibility(off, kf, K, rows), full[rows].astype(np.int32))


def test_hand_made_weights():
    off, kf, K, rows = WEIGHTS["hand_k5"]
    assert mr.covisibility(off, kf, K, rows).tolist() == mr.HAND_K5["weights"]
    off, kf, K, rows = WEIGHTS["column0"]
    assert (mr.covisibility(off, kf, K, np.array([0], np.int32))[0, 0]) == len(off) - 1
