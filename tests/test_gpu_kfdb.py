"""The keyframe database on the MI355X (ygz_hip_kfdb_*, ygz_slam_amd/csrc/kfdb.hip) through the C ABI against its restatement
tests/kfdb_ref.c, common words and scores bit for bit, on the smallest shapes at which the kernel can go wrong (the fixture of
tests/kfdb_ref.py): rows of 0, 1, 63, 64, 65, 128, 200 and 8192 words; databases of 1, 2, 64, 65 and 130 rows with dead rows at the first,
last and a middle position; add after erase, clear followed by add with the ids restarting; a growth step of the store crossed in
mid-sequence; queries of 0, 1, 65 and 8192 words; 1, 3 and 64 queries per call, each equal to the same queries asked one at a time; words up
to 2^31 - 1; a row identical to the query, a row sharing nothing with it, and a row whose only shared words sit in the last lane of one
64-word chunk and the first lane of the next; the row cap and the refusals through a live handle."""
import ctypes
import os
import re

import numpy as np
import pytest

import kfdb_ref as kr
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return kr.fixture()


@pytest.fixture()
def db(hip_lib, ctx):
    d = hip_lib.KeyframeDatabase(ctx)
    yield d
    d.close()


def _same(got, want, what):
    gc, gs = got
    wc, ws = want
    assert gc.shape == wc.shape and gs.shape == ws.shape, what
    bad = np.argwhere((gc != wc) | (kr.bits(gs) != kr.bits(ws)))
    assert len(bad) == 0, (what, bad[:5].tolist(), [(int(gc[tuple(b)]), int(wc[tuple(b)]), float(gs[tuple(b)]), float(ws[tuple(b)])) for b in bad[:5]])


def _fill(db, fx, n):
    for k in range(n):
        assert db.add(*fx["rows"][k]) == k
    assert db.info()[:2] == (n, n)


@pytest.mark.parametrize("n_rows", [1, 2, 64, 65, 130])
def test_database_sizes_with_dead_rows(db, fx, n_rows):
    _fill(db, fx, n_rows)
    q = fx["queries"][:4]
    want = kr.expected(fx, n_rows)
    _same(db.query(q), (want[0][:4], want[1][:4]), "all alive")
    dead = sorted({0, n_rows // 2, n_rows - 1})
    for e in dead:
        db.erase(e)
    db.erase(dead[0])                                                              # erasing a dead row: fine, nothing changes
    assert db.info()[:2] == (n_rows, n_rows - len(dead))
    want = kr.expected(fx, n_rows, dead=dead)
    got = db.query(q)
    _same(got, (want[0][:4], want[1][:4]), "dead rows")
    assert (got[0][:, dead] == -1).all() and (kr.bits(got[1][:, dead]) == 0).all()


def test_named_rows_and_queries(db, fx):
    """every named row length against every named query length, the identical row, the disjoint row, the chunk-edge row, the word 2^31 - 1"""
    _fill(db, fx, 14)
    common, score = db.query(fx["queries"][:5])
    want = kr.expected(fx, 14)
    _same((common, score), (want[0][:5], want[1][:5]), "named")
    assert common[0, 0] == 200 and common[0, 10] == 0 and common[0, 11] == 2 and common[0, 12] >= 1 and common[3, 1] > 4096
    assert (common[:, 2] == 0).all() and (kr.bits(score[:, 2]) == kr.bits(-0.0)).all()          # the empty row
    assert (common[4] == 0).all()                                                                # the empty query


@pytest.mark.parametrize("n_queries", [1, 3, 64])
def test_batches_equal_single_queries(db, fx, n_queries):
    _fill(db, fx, 130)
    db.erase(77)
    want = kr.expected(fx, 130, dead=(77,))
    got = db.query(fx["queries"][:n_queries])
    _same(got, (want[0][:n_queries], want[1][:n_queries]), "batch")
    for q in range(n_queries):
        one = db.query([fx["queries"][q]])
        assert np.array_equal(one[0][0], got[0][q]) and np.array_equal(kr.bits(one[1][0]), kr.bits(got[1][q])), q


def test_add_after_erase_and_clear_restarts_ids(db, fx):
    _fill(db, fx, 5)
    db.erase(1)
    assert db.add(*fx["rows"][20]) == 5                                            # ids are never reused
    rows = [0, 1, 2, 3, 4, 20]
    want_c, want_s = fx["common"][:3][:, rows].copy(), fx["score"][:3][:, rows].copy()
    want_c[:, 1], want_s[:, 1] = -1, 0.0
    _same(db.query(fx["queries"][:3]), (want_c, want_s), "add after erase")
    assert db.info() == (6, 5, sum(len(fx["rows"][k][0]) for k in rows))
    db.clear()
    assert db.info() == (0, 0, 0)
    for k, r in enumerate([30, 9, 31]):
        assert db.add(*fx["rows"][r]) == k                                         # ids restart at 0
    _same(db.query(fx["queries"][:3]), (fx["common"][:3][:, [30, 9, 31]], fx["score"][:3][:, [30, 9, 31]]), "after clear")


def test_growth_step_in_mid_sequence(db, fx):
    """8192-word rows until the store's first allocation is passed: the rows added before the step answer as they did, all match the restatement"""
    hip = open(os.path.join(ROOT, "ygz_slam_amd", "csrc", "kfdb.hip")).read()
    initial_units = int(re.search(r"#define\s+KFDB_INITIAL_UNITS\s+(\d+)", hip).group(1))
    big, q = fx["rows"][9], fx["queries"][1:4]
    assert len(big[0]) == 8192
    per_row = 8192 + 4096                                                          # 8-byte units: the weights, then the words
    before_n = initial_units // per_row
    assert 1 <= before_n <= 16
    order = [9, 1] * 8
    rows = order[:before_n]
    for r in rows:
        db.add(*fx["rows"][r])
    before = db.query(q)
    for r in order[before_n:before_n + 2]:                                         # these no longer fit the first allocation
        db.add(*fx["rows"][r])
        rows.append(r)
    assert db.info()[2] * 12 > initial_units * 8
    after = db.query(q)
    _same((after[0][:, :before_n], after[1][:, :before_n]), before, "rows before the step")
    _same(after, (fx["common"][1:4][:, rows], fx["score"][1:4][:, rows]), "after the step")


def test_row_cap_and_refusals_through_a_live_handle(hip_lib, db, fx):
    lib = hip_lib.load()
    INV, CAP = hip_lib.E_INVALID, hip_lib.E_CAPACITY
    off, word, weight = hip_lib.kfdb_pack(fx["queries"][:1])
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    c, s = np.zeros(8, np.int32), np.zeros(8)
    args = lambda: (off.ctypes.data_as(ip), word.ctypes.data_as(ip), weight.ctypes.data_as(dp), c.ctypes.data_as(ip), s.ctypes.data_as(dp))
    assert lib.ygz_hip_kfdb_query(db._db, 1, *args()) == INV                       # no rows yet
    assert lib.ygz_hip_kfdb_erase(db._db, 0) == INV and lib.ygz_hip_kfdb_erase(db._db, -1) == INV
    for k in range(hip_lib.KFDB_MAX_ENTRIES):                                      # empty rows: no upload
        assert db.add([], []) == k
    e = ctypes.c_int32(-7)
    assert lib.ygz_hip_kfdb_add(db._db, None, None, 0, ctypes.byref(e)) == CAP and e.value == -7
    db.erase(5)
    assert lib.ygz_hip_kfdb_add(db._db, None, None, 0, ctypes.byref(e)) == CAP     # ids are not reused: an erase frees no row
    assert db.info() == (hip_lib.KFDB_MAX_ENTRIES, hip_lib.KFDB_MAX_ENTRIES - 1, 0)
    common, score = db.query(fx["queries"][:2])                                    # 4096 rows, all empty, one dead
    assert (np.delete(common, 5, axis=1) == 0).all() and (common[:, 5] == -1).all()
    assert (kr.bits(np.delete(score, 5, axis=1)) == kr.bits(-0.0)).all() and (kr.bits(score[:, 5]) == 0).all()
    assert lib.ygz_hip_kfdb_erase(db._db, hip_lib.KFDB_MAX_ENTRIES) == INV
    db.clear()
    assert db.add(*fx["rows"][0]) == 0
