"""The projection-guided descriptor search on the MI355X (ygz_hip_search_by_projection / ygz_hip_projection_candidates,
ygz_slam_amd/csrc/proj.hip) against its restatement tests/proj_ref.c: match, dist, pred_level, counts and the candidate stage's lists bit for
bit.  Point counts around the wavefront and block width, keypoint counts around the LDS tile and at the capacity of 640x480, 1, 2 and 64
problems of mixed sizes in one call, claim on and off, with and without kp_taken / pt_normal / pt_skip, s = 1 and 1.2; the edge cases of every
cull on their exact limits; bad arguments and capacities are refused."""
import ctypes as C

import numpy as np
import pytest

import proj_ref as pr

pytestmark = pytest.mark.gpu

N_PT = [1, 63, 64, 65, 1000, 5000]
N_KP = [1, 255, 256, 257, 3072]
KX = np.array([512.0, 512.0, 320.0, 240.0])          # intrinsics whose products are exact, for the cases on a limit
IDENT = [0, 0, 0, 1, 0, 0, 0, 1.0]


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = hip_lib.HipContext(width=640, height=480, levels=3, max_frames=2)
    assert c.cells == 3072
    yield c
    c.close()


def _same(ctx, problems, K4=pr.K4_DEFAULT, **kw):
    """the fused call (claim as given) and, per problem, the candidate stage, against the restatement; returns the device's result"""
    ref = pr.search(problems, K4=K4, **kw)
    out = ctx.search_by_projection(problems, K4, **kw)
    for k in ("pred_level", "match", "dist", "counts"):
        assert np.array_equal(out[k], ref[k]), (k, np.nonzero(np.asarray(out[k]) != ref[k])[0][:8])
    return out


def _same_lists(ctx, sc, K4=pr.K4_DEFAULT, **kw):
    kw.pop("claim", None)
    ref = pr.candidates(sc, K4=K4, **kw)
    out = ctx.projection_candidates(sc, K4, **kw)
    for k in ("pred_level", "n_cand", "cand_idx", "cand_dist"):
        assert np.array_equal(out[k], ref[k]), (k, np.nonzero(np.asarray(out[k]) != ref[k])[0][:8])
    return out


@pytest.mark.parametrize("n_kp", N_KP)
@pytest.mark.parametrize("n_pt", N_PT)
def test_device_equals_the_restatement(ctx, n_pt, n_kp):
    v = N_PT.index(n_pt) * len(N_KP) + N_KP.index(n_kp)          # the options cycle over the 30 shapes: every combination of each pair occurs
    sc = pr.scene(n_pt, n_kp, 100 + v, s=1.2 if v & 1 else 1.0, normals=bool(v & 2), taken=bool(v & 4), skip=bool((v >> 3) & 1))
    th, th_dist = ((10.0, 50), (7.5, 100), (4.0, 256))[v % 3]
    lists = _same_lists(ctx, sc, th=th, th_dist=th_dist)
    a = _same(ctx, [sc], th=th, th_dist=th_dist, claim=0)
    b = _same(ctx, [sc], th=th, th_dist=th_dist, claim=1)
    if n_pt >= 1000 and n_kp >= 255:
        assert lists["n_cand"].max() >= 1 and 0 < b["counts"][0, 0] <= a["counts"][0, 0]
        hit = b["match"][b["match"] >= 0]
        assert len(set(hit.tolist())) == len(hit)


@pytest.mark.parametrize("P", [2, 64])
def test_many_problems_equal_the_restatement(ctx, P):
    rng = np.random.default_rng(P)
    sizes = [(5000, 3072), (65, 257)] if P == 2 else [(int(rng.choice([1, 63, 64, 65, 257, 1000])), int(rng.choice(N_KP))) for _ in range(P)]
    scs = [pr.scene(n, k, 700 + 7 * q, s=1.2 if q % 3 == 0 else 1.0, normals=q % 2 == 0, taken=q % 4 == 1, skip=q % 5 == 2)
           for q, (n, k) in enumerate(sizes)]
    for claim in (0, 1):
        out = _same(ctx, scs, claim=claim)
        assert (out["counts"][:, 0] > 0).sum() >= P // 2


def _axis_case(z, dmax, kp_px=((320.0, 240.0),), pw=None):
    d = np.random.default_rng(4).integers(0, 256, 32).astype(np.uint8)
    pw = [[0, 0, zz] for zz in z] if pw is None else pw
    n = len(pw)
    return dict(kp_px=np.array(kp_px), kp_level=np.zeros(len(kp_px), np.int32), kp_desc=np.tile(d, (len(kp_px), 1)), pw=pw,
                pt_desc=np.tile(d, (n, 1)), pt_dmax=np.broadcast_to(dmax, n).copy(), S=IDENT)


def test_points_on_the_limits(ctx):
    # z <= 0
    out = _same(ctx, [_axis_case([0.0, -3.0, 4.0], 4.0)], K4=KX, claim=0)
    assert out["pred_level"].tolist() == [-1, -1, 0] and out["match"].tolist() == [-1, -1, 0]
    # u exactly 0 (kept) and exactly the width (culled); v exactly 0 and exactly the height
    pw = [[-1.25, 0, 2.0], [1.25, 0, 2.0], [0, -0.9375, 2.0], [0, 0.9375, 2.0]]
    sc = _axis_case(None, [np.sqrt(1.25 ** 2 + 4), np.sqrt(1.25 ** 2 + 4), np.sqrt(0.9375 ** 2 + 4), np.sqrt(0.9375 ** 2 + 4)],
                    kp_px=((0.0, 240.0), (639.5, 240.0), (320.0, 0.0), (320.0, 479.5)), pw=pw)
    assert pr.candidates(sc, K4=KX)["uv"].tolist() == [[0, 240], [0, 0], [320, 0], [0, 0]]
    out = _same(ctx, [sc], K4=KX, claim=0)
    assert out["pred_level"].tolist() == [0, -1, 0, -1] and out["match"].tolist() == [0, -1, 2, -1]
    # d exactly on both range limits (kept) and one step beyond (culled)
    dmax = 5.0
    hi, lo = 1.2 * dmax, 0.8 * (dmax / 4)
    out = _same(ctx, [_axis_case([hi, np.nextafter(hi, 9), lo, np.nextafter(lo, 0)], dmax)], K4=KX, claim=0)
    assert out["pred_level"].tolist() == [0, -1, 2, -1]
    # the window is open: a keypoint exactly r away is no candidate, one step inside is
    sc = _axis_case([4.0], 4.0, kp_px=((330.0, 240.0), (320.0, 250.0), (np.nextafter(330.0, 0), np.nextafter(230.0, 999))))
    out = _same_lists(ctx, sc, K4=KX)
    assert out["n_cand"].tolist() == [1] and out["cand_idx"][0, 0] == 2


def test_empty_window_duplicates_and_a_claim_chain(ctx):
    sc = _axis_case([4.0], 4.0, kp_px=((100.0, 100.0), (500.0, 400.0)))
    out = _same(ctx, [sc], K4=KX)
    assert out["pred_level"].tolist() == [0] and out["match"].tolist() == [-1] and out["dist"].tolist() == [-1] and out["counts"].tolist() == [[0, 0]]
    # duplicate descriptors: the smaller index
    sc = _axis_case([4.0], 4.0, kp_px=((900.0, 0.0), (322.0, 240.0), (318.0, 241.0)))
    assert _same(ctx, [sc], K4=KX)["match"].tolist() == [1]
    # 40 points contend for 3 keypoints: the first three get them in index order of their lists, the rest nothing
    sc = _axis_case([4.0 + 0.01 * i for i in range(40)], 4.5, kp_px=((321.0, 240.0), (319.0, 241.0), (320.0, 238.0)))
    rng = np.random.default_rng(8)
    for j in range(3):
        sc["kp_desc"][j] = pr.flip_bits(rng, sc["kp_desc"][j], 3 * (2 - j))        # keypoint 2 is the best, then 1, then 0
    out = _same(ctx, [sc], K4=KX, claim=1)
    assert out["match"].tolist() == [2, 1, 0] + [-1] * 37 and out["counts"].tolist() == [[3, 0]]
    assert _same(ctx, [sc], K4=KX, claim=0)["match"].tolist() == [2] * 40
    lists = _same_lists(ctx, sc, K4=KX)
    assert (lists["n_cand"] == 3).all() and (lists["cand_idx"][:, :3] == [2, 1, 0]).all()


def test_overflow_truncates_as_specified(ctx):
    d = np.random.default_rng(9).integers(0, 256, 32).astype(np.uint8)
    kp = [(316.0 + j, 240.0) for j in range(9)]
    sc = _axis_case([4.0] * 10, 4.0, kp_px=kp)
    lists = _same_lists(ctx, sc, K4=KX)
    assert (lists["n_cand"] == 9).all() and lists["cand_idx"][0].tolist() == list(range(8))
    out = _same(ctx, [sc], K4=KX, claim=1)
    assert out["match"].tolist() == list(range(8)) + [-1, -1] and out["counts"].tolist() == [[8, 10]]
    # the last keypoint is the closest: it enters the full list at its head
    sc["kp_desc"][:8] = pr.flip_bits(np.random.default_rng(1), sc["kp_desc"][0], 5)
    lists = _same_lists(ctx, sc, K4=KX)
    assert lists["cand_idx"][0].tolist() == [8, 0, 1, 2, 3, 4, 5, 6] and lists["cand_dist"][0].tolist() == [0] + [5] * 7
    _same(ctx, [sc], K4=KX, claim=1)


def test_every_point_culled(ctx):
    sc = pr.scene(300, 257, 21, skip=True)
    sc["pt_skip"][:] = 1
    behind = pr.scene(70, 64, 22)
    behind["pw"] = (np.array([[0, 0, -5.0]]) - behind["S"][4:7]) @ pr.quat_to_R(behind["S"][:4]) + np.zeros((70, 1))
    for claim in (0, 1):
        out = _same(ctx, [sc, behind], claim=claim)
        assert (out["match"] == -1).all() and (out["dist"] == -1).all() and (out["pred_level"] == -1).all() and not out["counts"].any()


def test_bad_arguments_and_capacities_are_refused(ctx, hip_lib):
    sc = pr.scene(50, 40, 5)

    def code(problems, **kw):
        with pytest.raises(hip_lib.YgzHipError) as e:
            ctx.search_by_projection(problems, pr.K4_DEFAULT, **kw)
        return e.value.code
    assert code([sc] * 65) == hip_lib.E_CAPACITY
    big = pr.scene(4, ctx.cells + 1, 6)
    assert code([sc, big]) == hip_lib.E_CAPACITY
    many = dict(sc, pw=np.zeros((32769, 3)), pt_desc=np.zeros((32769, 32), np.uint8), pt_dmax=np.ones(32769), pt_normal=None)
    assert code([many, many]) == hip_lib.E_CAPACITY
    assert code([]) == hip_lib.E_INVALID
    for kw in (dict(th=0.0), dict(th=-1.0), dict(th=float("nan")), dict(th_dist=-1), dict(th_dist=257)):
        assert code([sc], **kw) == hip_lib.E_INVALID, kw
    for name in ("kp_px", "kp_level", "kp_desc", "pw", "pt_desc", "pt_dmax"):
        assert code([sc, dict(sc, **{name: None}, n_kp=40, n_pt=50)]) == hip_lib.E_INVALID, name
    assert code([dict(sc, n_kp=0)]) == hip_lib.E_INVALID and code([dict(sc, n_pt=0)]) == hip_lib.E_INVALID
    for S in ([0, 0, 0, 1, 0, 0, 0, 0.0], [0, 0, 0, 1, 0, 0, 0, -1.0], [0, 0, 0, 1, 0, float("inf"), 0, 1.0], [float("nan"), 0, 0, 1, 0, 0, 0, 1.0]):
        assert code([dict(sc, S=S)]) == hip_lib.E_INVALID, S
    # a null context, a null problem array, a null K4: straight through the C ABI
    lib = hip_lib.load()
    arr, keep = hip_lib.proj_problems([sc])
    K = (C.c_double * 4)(*pr.K4_DEFAULT)
    lib.ygz_hip_search_by_projection.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * 4
    assert lib.ygz_hip_search_by_projection(None, 1, arr, K, None, None, None, None, None) == hip_lib.E_INVALID
    assert lib.ygz_hip_search_by_projection(ctx._ctx, 1, None, K, None, None, None, None, None) == hip_lib.E_INVALID
    assert lib.ygz_hip_search_by_projection(ctx._ctx, 1, arr, None, None, None, None, None, None) == hip_lib.E_INVALID
    lib.ygz_hip_projection_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * 4
    assert lib.ygz_hip_projection_candidates(ctx._ctx, None, K, None, None, None, None, None) == hip_lib.E_INVALID
    # every output may be NULL, params NULL are the defaults: the call still runs
    assert lib.ygz_hip_search_by_projection(ctx._ctx, 1, arr, K, None, None, None, None, None) == 0
    # ... and the context still works afterwards
    _same(ctx, [sc])
