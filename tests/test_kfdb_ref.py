"""The restatement of the keyframe database's query (tests/kfdb_ref.c) held to two witnesses written differently: numpy on dense vectors
(np.intersect1d for the common words, 1 - 0.5 |a - b|_1 for the score of L1-normalised vectors, within 1e-12) and a pure-Python float loop
over the sorted shared words (bit for bit).  It also shows that the fixture of tests/test_gpu_kfdb.py has teeth: for some of its (query, row)
pairs a pairwise-tree sum of the same terms differs from the sequential sum in its last bits, so a kernel that reduced in parallel would fail
the bit comparison there.  CPU only."""
import math

import numpy as np

import kfdb_ref as kr


def _python_score(q, r):
    """DBoW3::L1Scoring::score as a float loop over the sorted shared words"""
    qw, rw = dict(zip(q[0].tolist(), q[1].tolist())), dict(zip(r[0].tolist(), r[1].tolist()))
    s = 0.0
    n = 0
    for word in sorted(set(qw) & set(rw)):
        v, w = qw[word], rw[word]
        s += math.fabs(v - w) - math.fabs(v) - math.fabs(w)
        n += 1
    return n, -s / 2.0


def test_first_witness_numpy_on_dense_normalised_vectors():
    rng = np.random.default_rng(5)
    universe = np.arange(3000)
    vecs = []
    for n in [1, 2, 63, 64, 65, 200, 700, 1500]:
        w, v = kr.vector(rng, universe, n)
        vecs.append((w, v / v.sum()))
    common, score = kr.query(vecs, np.ones(len(vecs), np.uint8), vecs)
    dense = np.zeros((len(vecs), 3000))
    for k, (w, v) in enumerate(vecs):
        dense[k, w] = v
    for q in range(len(vecs)):
        for e in range(len(vecs)):
            assert common[q, e] == len(np.intersect1d(vecs[q][0], vecs[e][0]))
            assert abs(score[q, e] - (1.0 - 0.5 * np.abs(dense[q] - dense[e]).sum())) < 1e-12, (q, e)
    assert np.allclose(np.diag(score), 1.0, atol=1e-12) and (np.diag(common) == [len(w) for w, _ in vecs]).all()


def test_second_witness_python_float_loop_bit_for_bit():
    fx = kr.fixture()
    rows, queries = fx["rows"], fx["queries"]
    pairs = [(q, e) for q in range(6) for e in range(14)] + [(q, e) for q in range(6, 64, 7) for e in range(14, 130, 9)]
    for q, e in pairs:
        n, s = _python_score(queries[q], rows[e])
        assert n == fx["common"][q, e], (q, e)
        assert (kr.bits(s) == kr.bits(fx["score"][q, e])).all(), (q, e, s, fx["score"][q, e])


def test_dead_rows_and_empty_vectors():
    fx = kr.fixture()
    alive = np.ones(14, np.uint8)
    alive[[0, 5, 13]] = 0
    common, score = kr.query(fx["rows"][:14], alive, fx["queries"][:5])
    ec, es = kr.expected(fx, 14, dead=(0, 5, 13))
    assert np.array_equal(common, ec[:5]) and np.array_equal(kr.bits(score), kr.bits(es[:5]))
    assert (common[:, [0, 5, 13]] == -1).all() and (kr.bits(score[:, [0, 5, 13]]) == 0).all()
    # the empty row (rows[2]) and the empty query (queries[4]) share nothing: -0.0 / 2, as Vocabulary::score returns it
    assert (fx["common"][:, 2] == 0).all() and (fx["common"][4] == 0).all()
    assert (kr.bits(fx["score"][4]) == kr.bits(-0.0)).all()


def test_fixture_covers_the_named_shapes():
    fx = kr.fixture()
    rows, queries = fx["rows"], fx["queries"]
    assert len(rows) == 130 and len(queries) == 64
    assert [len(w) for w, _ in rows[2:10]] == list(kr.ROW_LENGTHS) and len(rows[1][0]) == 8192
    assert [len(w) for w, _ in queries[1:4]] == list(kr.QUERY_LENGTHS) and len(queries[4][0]) == 0
    for w, v in rows + queries:
        assert (np.diff(w.astype(np.int64)) > 0).all() and (w >= 0).all() and np.isfinite(v).all() and (v > 0).all()
    q0 = queries[0]
    assert np.array_equal(rows[0][0], q0[0]) and np.array_equal(rows[0][1], q0[1]) and fx["common"][0, 0] == 200
    assert fx["common"][0, 10] == 0                                                  # shares nothing
    shared = np.flatnonzero(np.isin(rows[11][0], q0[0]))
    assert shared.tolist() == [63, 64] and fx["common"][0, 11] == 2                  # the last lane of one chunk, the first of the next
    assert rows[12][0][-1] == kr.WORD_MAX == q0[0][-1] and fx["common"][0, 12] >= 1   # words up to 2^31 - 1
    assert fx["common"][3, 1] > 4096                                                 # the 8192-word query against the 8192-word row
    w = np.concatenate([v for _, v in rows])
    assert w.min() < 1e-8 and w.max() > 0.1                                          # weights over several decades


def test_fixture_tells_a_tree_sum_from_the_sequential_sum():
    fx = kr.fixture()
    differ = 0
    for q, e in [(0, 0), (3, 1), (2, 1), (3, 9), (0, 1), (3, 8)]:
        t = kr.tree_score(fx["queries"][q], fx["rows"][e])
        assert abs(t - fx["score"][q, e]) <= 1e-9 * max(1.0, abs(t))                 # the same terms
        differ += int((kr.bits(t) != kr.bits(fx["score"][q, e])).any())
    assert differ >= 1
    # and the tree function itself is right where the order cannot matter: one shared term, none
    assert (kr.bits(kr.tree_score(fx["queries"][0], fx["rows"][10])) == kr.bits(fx["score"][0, 10])).all()
    one = [(q, e) for q in range(64) for e in range(130) if fx["common"][q, e] == 1][0]
    assert (kr.bits(kr.tree_score(fx["queries"][one[0]], fx["rows"][one[1]])) == kr.bits(fx["score"][one])).all()
