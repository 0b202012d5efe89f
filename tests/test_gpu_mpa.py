"""Map-point attributes on the MI355X (ygz_slam_amd/csrc/mpa.hip: k_mpa_attr) against tests/mpa_ref.c: every double of every point is
bit-identical (compared as its 64 bits), every state exact, no point left out.  One small context serves every case, so the packed block's
scratch buffer is reused from call to call, by smaller and by larger maps."""
import numpy as np
import pytest

import mpa_ref as mr
from conftest import make_ctx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = make_ctx(hip_lib, width=320, height=240, levels=3, max_frames=2)
    yield c
    c.close()


def both(ctx, m):
    got = ctx.map_point_attributes(m["center"], m["pw"], m["off"], m["kf"], m["level"])
    mr.same(got, mr.attributes(m))
    return got


@pytest.mark.parametrize("K", (1, 4096))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 257, 1025))
def test_wavefront_and_block_edges(ctx, P, K):
    rows = np.random.default_rng(P).integers(1, 9, P)
    got = both(ctx, mr.make_map(K, rows, 100 + P + K))
    assert (got["state"] == 1).all() and (got["dmax"] > 0).all()


def test_ragged_rows_with_0_and_256_in_one_wavefront(ctx):
    m = mr.make_map(37, mr.ragged_rows(300, 4), 5)
    got = both(ctx, m)
    rows = np.diff(m["off"])
    assert rows[:7].tolist() == [0, 256, 1, 255, 2, 256, 0] and (got["state"] == (rows > 0)).all()
    assert (got["dmax"][rows == 0] == 0).all() and (got["normal"][rows == 0] == 0).all()
    both(ctx, mr.make_map(3, np.zeros(70, np.int64), 6))                   # a map without a single row


def test_degenerate_points(ctx):
    m, states = mr.degenerate_map()
    got = both(ctx, m)
    assert got["state"].tolist() == states and np.isfinite(got["dmax"]).all() and np.isfinite(got["normal"]).all()
    off = got["state"] != 1
    assert (got["dmax"][off] == 0).all() and (got["normal"][off] == 0).all()


def test_second_call_with_a_smaller_map_reuses_the_scratch(ctx):
    big, small = mr.make_map(200, mr.ragged_rows(5000, 7), 8), mr.make_map(5, mr.ragged_rows(90, 9), 10)
    a = both(ctx, big)
    b = both(ctx, small)
    mr.same(both(ctx, big), a)
    mr.same(both(ctx, small), b)


def test_refusals_through_a_live_context(ctx, hip_lib):
    E = hip_lib.YgzHipError
    m = mr.make_map(4, [2, 0, 3], 11)

    def code(**kw):
        a = dict(m, **kw)
        with pytest.raises(E) as e:
            ctx.map_point_attributes(a["center"], a["pw"], a["off"], a["kf"], a["level"])
        return e.value.code
    CAP, INV = hip_lib.E_CAPACITY, hip_lib.E_INVALID
    assert code(center=np.zeros((hip_lib.MAP_MAX_KEYFRAMES + 1, 3))) == CAP
    P = hip_lib.MPA_MAX_POINTS + 1
    assert code(pw=np.ones((P, 3)), off=np.zeros(P + 1, np.int32), kf=[], level=[]) == CAP
    n = hip_lib.MAP_MAX_OBS_PER_POINT + 1
    assert code(pw=np.ones((1, 3)), off=[0, n], kf=np.zeros(n, np.int32), level=np.zeros(n, np.int32)) == CAP
    # too many rows in the call: 4097 points of 256 rows
    P, n = hip_lib.MAP_MAX_OBS // 256 + 1, hip_lib.MAP_MAX_OBS + 256
    assert code(pw=np.ones((P, 3)), off=np.arange(P + 1, dtype=np.int32) * 256, kf=np.zeros(n, np.int32), level=np.zeros(n, np.int32)) == CAP
    assert code(kf=[0, 4, 1, 2, 3]) == INV and code(kf=[0, -1, 1, 2, 3]) == INV and code(level=[0, 31, 0, 0, 0]) == INV
    assert code(off=[0, 3, 2, 5]) == INV and code(off=[1, 2, 2, 5]) == INV
    bad = m["pw"].copy()
    bad[1, 2] = np.nan
    assert code(pw=bad) == INV
    bad = m["center"].copy()
    bad[3, 0] = np.inf
    assert code(center=bad) == INV
    both(ctx, m)                                                          # the context is none the worse for it
    lim = mr.make_map(2, np.full(hip_lib.MAP_MAX_OBS // 256, 256), 12, levels=(0, 30))     # the limit itself: 4096 points of 256 rows
    assert (both(ctx, lim)["state"] == 1).all()
