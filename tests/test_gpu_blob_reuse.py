"""The packed-block helper (ygz_blob_open / ygz_blob_upload / ygz_blob_fetch, ygz_slam_amd/csrc/ctx.hip) handing out memory that was used
before, on ONE context: a scratch buffer that has to grow and a 1 MiB staging arena that wraps.  A small call, then larger calls in a row,
then the small call again, every output compared bit for bit with the restatements tests/cull_ref.c and tests/kfdb_ref.c.

  culling   the 2-point, 3-keyframe OK_CASE of tests/test_cull_surface_build.py; then 4096 points x 8 observations over 64 keyframes, every
            keyframe a candidate, four times in a row (ygz_hip_keyframe_redundancy stages 0.27 MB and ygz_hip_cull_keyframes 0.44 MB per call:
            the arena wraps at least twice, the scratch buffer grows once); then the 2-point case again
  database  1 query against 2 rows; 8 queries against 2048 rows of 64 words; 1 query against the 2 rows again

No larger shapes: the point is the reallocation and the wrap, not the load."""
import numpy as np
import pytest

import cull_ref as cr
import kfdb_ref as kr
from test_cull_surface_build import OK_CASE

pytestmark = pytest.mark.gpu

WALK_KEYS = ["culled", "tracked", "redundant", "point_dead"]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    yield c
    c.close()


def _large_cull_case():
    rng = np.random.default_rng(4096)
    P, per, K = 4096, 8, 64
    kf = np.sort(np.argsort(rng.random((P, K)), axis=1)[:, :per], axis=1).astype(np.int32).reshape(-1)      # 8 distinct keyframes per point, ascending
    return dict(offsets=np.arange(0, P * per + 1, per, dtype=np.int32), kf=kf, level=rng.integers(0, 8, P * per).astype(np.int32), K=K,
                cand=rng.permutation(K).astype(np.int32))


@pytest.fixture(scope="module")
def cull_cases():
    """(case, the restatement's counts, the restatement's walk) for the small and the large case, computed once"""
    out = {}
    for name, c in [("small", OK_CASE), ("large", _large_cull_case())]:
        out[name] = (c, cr.redundancy(c["offsets"], c["kf"], c["level"], c["K"]), cr.cull(c["offsets"], c["kf"], c["level"], c["K"], c["cand"]))
    return out


def _check_cull(ctx, entry, what):
    c, want_counts, want_walk = entry
    got = ctx.keyframe_redundancy(c["offsets"], c["kf"], c["level"], c["K"])
    for k in ["tracked", "redundant"]:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want_counts[k]), (what, k)
    got = ctx.cull_keyframes(c["offsets"], c["kf"], c["level"], c["K"], c["cand"])
    for k in WALK_KEYS:
        assert got[k].dtype == want_walk[k].dtype and np.array_equal(got[k], want_walk[k]), (what, k)


def test_culling_small_large_small_on_one_context(ctx, cull_cases):
    large = cull_cases["large"]
    assert large[2]["culled"].sum() > 0 and large[1]["redundant"].sum() > 0            # the large case decides something
    _check_cull(ctx, cull_cases["small"], "small, first")
    for k in range(4):
        _check_cull(ctx, large, "large, call %d" % k)
    _check_cull(ctx, cull_cases["small"], "small, again")


def _check_query(db, rows, queries, what):
    common, score = db.query(queries)
    want_common, want_score = kr.query(rows, np.ones(len(rows), np.uint8), queries)
    assert common.shape == want_common.shape and np.array_equal(common, want_common), what
    assert np.array_equal(kr.bits(score), kr.bits(want_score)), what


def test_database_query_small_large_small_on_one_context(hip_lib, ctx):
    rng = np.random.default_rng(2048)
    rows = [kr.vector(rng, 4096, 64) for _ in range(2048)]
    queries = [kr.vector(rng, 4096, 64) for _ in range(8)]
    small, large = hip_lib.KeyframeDatabase(ctx), hip_lib.KeyframeDatabase(ctx)
    try:
        for k, r in enumerate(rows[:2]):
            assert small.add(*r) == k
        for k, r in enumerate(rows):
            assert large.add(*r) == k
        _check_query(small, rows[:2], queries[:1], "1 query against 2 rows, first")
        _check_query(large, rows, queries, "8 queries against 2048 rows")
        _check_query(small, rows[:2], queries[:1], "1 query against 2 rows, again")
    finally:
        small.close()
        large.close()
