"""ctypes loader of tests/kfdb_ref.c, the restatement of the keyframe database's query (ygz_slam_amd/csrc/kfdb.hip) that
tests/test_kfdb_ref.py and tests/test_gpu_kfdb.py hold ygz_hip_kfdb_query against.  Test infrastructure: compiled with gcc into a temporary
directory the first time it is used, never imported by the package.  Also the seeded vectors of those tests and of tools/kfdb_bench.py."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

MAX_ENTRIES, MAX_WORDS, MAX_QUERIES = 4096, 8192, 64
WORD_MAX = 2 ** 31 - 1
ROW_LENGTHS = (0, 1, 63, 64, 65, 128, 200, 8192)          # the row lengths the issue names
QUERY_LENGTHS = (1, 65, 8192)


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="kfdb_ref_")
        so = os.path.join(d, "libkfdb_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "kfdb_ref.c"), "-lm"])
        _lib = ctypes.CDLL(so)
        _lib.kfdb_ref_tree_score.restype = ctypes.c_double
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def pack(vectors):
    """a list of (word, weight) as CSR: offsets [n + 1] int32, word int32, weight float64 (each of at least one element)"""
    off = np.zeros(len(vectors) + 1, np.int32)
    off[1:] = np.cumsum([len(w) for w, _ in vectors])
    word = np.ascontiguousarray(np.concatenate([np.asarray(w, np.int32).reshape(-1) for w, _ in vectors] + [np.zeros(1, np.int32)]))
    weight = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).reshape(-1) for _, v in vectors] + [np.zeros(1)]))
    return off, word, weight


def query(rows, alive, queries):
    """the restatement: common [n_queries][n_rows] int32, score [n_queries][n_rows] float64"""
    r_off, r_word, r_weight = pack(rows)
    q_off, q_word, q_weight = pack(queries)
    alive = np.ascontiguousarray(alive, np.uint8)
    assert len(alive) == len(rows)
    common, score = np.zeros((len(queries), len(rows)), np.int32), np.zeros((len(queries), len(rows)), np.float64)
    i32, f64 = ctypes.c_int32, ctypes.c_double
    lib().kfdb_ref_query(len(rows), _p(r_off, i32), _p(alive, ctypes.c_uint8), _p(r_word, i32), _p(r_weight, f64), len(queries), _p(q_off, i32),
                         _p(q_word, i32), _p(q_weight, f64), _p(common, i32), _p(score, f64))
    return common, score


def tree_score(a, b):
    """score of the pair with the shared words' terms summed as a pairwise tree"""
    aw, av = np.ascontiguousarray(a[0], np.int32), np.ascontiguousarray(a[1], np.float64)
    bw, bv = np.ascontiguousarray(b[0], np.int32), np.ascontiguousarray(b[1], np.float64)
    work = np.zeros(max(1, min(len(aw), len(bw))))
    return lib().kfdb_ref_tree_score(_p(aw, ctypes.c_int32), _p(av, ctypes.c_double), len(aw), _p(bw, ctypes.c_int32), _p(bv, ctypes.c_double),
                                     len(bw), _p(work, ctypes.c_double))


def weights(rng, n):
    """n weights over nine decades, 1e-9 .. 1: a sum of them depends on its order in the last bits"""
    return 10.0 ** rng.uniform(-9.0, 0.0, n)


def vector(rng, universe, n):
    """n distinct words of `universe` ascending, with weights()"""
    w = np.sort(rng.choice(universe, n, replace=False)).astype(np.int32)
    return w, weights(rng, n)


@functools.lru_cache(maxsize=None)
def fixture():
    """the rows and queries of the GPU tests (and of the CPU test that shows they have teeth): dict(rows [130], queries [64], expected of all
    rows alive: common, score).  Words come from 12000 ids spread over [0, 2^31 - 1], both ends included.
      rows[0]  identical to queries[0] (200 words)          rows[1]  8192 words
      rows[2 .. 9]  the lengths of ROW_LENGTHS              rows[10] shares nothing with queries[0]
      rows[11] 130 words, of which only number 63 and number 64 are words of queries[0]: the last lane of one chunk, the first of the next
      rows[12] ends with the word 2^31 - 1, as queries[0] does
      the rest 1 .. 300 words at random
      queries[0] 200 words; queries[1 .. 3] the lengths of QUERY_LENGTHS; queries[4] empty; the rest 1 .. 300 words"""
    rng = np.random.default_rng(20261018)
    universe = np.unique(np.concatenate([[0, WORD_MAX], rng.integers(0, WORD_MAX, 12000)])).astype(np.int64)
    inner = universe[:-1]
    q0w = np.sort(np.concatenate([rng.choice(inner, 199, replace=False), [WORD_MAX]])).astype(np.int32)
    q0 = (q0w, weights(rng, 200))
    rest = np.setdiff1d(universe, q0w)
    rows = [(q0w.copy(), q0[1].copy()), vector(rng, universe, 8192)]
    rows += [vector(rng, universe, n) for n in ROW_LENGTHS]
    rows.append(vector(rng, rest, 150))
    # 130 words: 63 foreign words below q0w[50], q0w[50], q0w[51], 65 foreign words above q0w[51]
    lo, hi = rest[rest < q0w[50]], rest[rest > q0w[51]]
    edge = np.concatenate([np.sort(rng.choice(lo, 63, replace=False)), q0w[50:52], np.sort(rng.choice(hi, 65, replace=False))]).astype(np.int32)
    rows.append((edge, weights(rng, 130)))
    last = np.sort(np.concatenate([rng.choice(inner, 40, replace=False), [WORD_MAX]])).astype(np.int32)
    rows.append((last, weights(rng, 41)))
    while len(rows) < 130:
        rows.append(vector(rng, universe, int(rng.integers(1, 301))))
    queries = [q0] + [vector(rng, universe, n) for n in QUERY_LENGTHS] + [(np.zeros(0, np.int32), np.zeros(0))]
    while len(queries) < 64:
        queries.append(vector(rng, universe, int(rng.integers(1, 301))))
    common, score = query(rows, np.ones(len(rows), np.uint8), queries)
    for a in (common, score):
        a.setflags(write=False)
    return dict(rows=rows, queries=queries, common=common, score=score)


def expected(fx, n_rows, dead=()):
    """the fixture's reference for the database of its first n_rows rows with the rows of `dead` erased"""
    common, score = fx["common"][:, :n_rows].copy(), fx["score"][:, :n_rows].copy()
    for e in dead:
        common[:, e], score[:, e] = -1, 0.0
    return common, score


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def synthetic(rng, n_vectors, n_words=1000, space=10 ** 6, skew=0.9):
    """BoW-like vectors for the benchmark: about n_words distinct words of a `space`-word vocabulary drawn with a Zipf-like frequency (rank r
    with probability ~ r^-skew over a random permutation of the ids), L1-normalised TF-IDF-like weights"""
    p = np.arange(1, space + 1, dtype=np.float64) ** -skew
    cdf = np.cumsum(p / p.sum())
    perm = rng.permutation(space)
    out = []
    for _ in range(n_vectors):
        draws = perm[np.minimum(np.searchsorted(cdf, rng.random(4 * n_words)), space - 1)]
        _, first = np.unique(draws, return_index=True)
        ids = np.sort(draws[np.sort(first)[:n_words]]).astype(np.int32)           # the first n_words distinct draws
        w = rng.gamma(2.0, 1.0, len(ids)) + 1e-3
        out.append((ids, w / w.sum()))
    return out
