"""The crafted limit cases of tests/depth_limit_cases.py on the MI355X: k_smap_pairs through ygz_hip_stereo_create_map_points
(ygz_slam_amd/csrc/smap.hip) and k_stereo_match / k_stereo_median through ygz_hip_stereo_match and ygz_hip_stereo_candidates
(csrc/stereo.hip).  Every case puts one input ON a limit of a rule of DESIGN.md sections 19 and 24 (a), or one np.nextafter step beyond
it, with everything exact in FP64.  For every case: every output of the device is equal to the restatement (tests/smap_ref.c,
tests/stereo_ref.c) bit for bit, and the case's LITERAL expectation holds on the device's output.

Pairs: every case alone, at index 0, 63, 64 and 256 of a problem of 257 pairs whose other pairs end with another, known code (wavefront,
ragged end), and as problem 0, 15 and 31 of a call of 32 problems with empty problems next to it and other cameras in every other problem
(the offsets table's lookup).  The cases of one parameter set share calls of up to 32 problems.  Depths: one call of each entry point per
case -- the median is a statistic of the call, so cases do not share one -- on a 320 x 240 context of three levels that holds the zero
pictures and the two designed ones.  No case is skipped and no comparison has a tolerance; tests/test_depth_limit_cases.py shows on the
CPU that the cases separate every wrong variant of every rule."""
import numpy as np
import pytest

import depth_limit_cases as dlc
import smap_ref as sm
import stereo_ref as sr
from conftest import make_ctx

pytestmark = pytest.mark.gpu


# ---- pairs -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_ctx(hip_lib):
    c = make_ctx(hip_lib, width=320, height=240, levels=3, max_frames=2, intrinsics=dlc.KP)
    yield c
    c.close()


def create(ctx, case, problems):
    """one call on the device and on the restatement: code, method and pos_world equal bit for bit, the counts equal"""
    got = ctx.stereo_create_map_points(problems, case.K4, **case.params)
    want = [sm.create(pb, case.K4, sm.default_params(**case.params)) for pb in problems]
    for k, name in enumerate(("code", "method", "pos_world")):
        assert dlc.equal_bits(got[name], np.concatenate([w[k] for w in want])) and len(got[name]) == sum(pb["n"] for pb in problems), (case.name, name)
    assert np.array_equal(got["counts"], [[int((w[0] == 0).sum()), int(((w[0] == 0) & (w[1] == 1)).sum())] for w in want])
    assert np.array_equal(got["offsets"], np.cumsum([0] + [pb["n"] for pb in problems]))
    return got


def test_every_pair_alone_and_at_every_index_of_257(pair_ctx):
    seen, largest = 0, 0
    for fam in dlc.pair_families(dlc.pair_cases()):
        entries = [(c, pos, c.pb if pos is None else dlc.pair_at(c, pos)) for c in fam for pos in (None,) + dlc.PAIR_POSITIONS]
        for at in range(0, len(entries), dlc.N_PROBLEMS):
            chunk = entries[at:at + dlc.N_PROBLEMS]
            got = create(pair_ctx, fam[0], [pb for _, _, pb in chunk])
            for q, (c, pos, pb) in enumerate(chunk):
                o, i = int(got["offsets"][q]), pos or 0
                assert dlc.pair_holds(c, got["code"][o + i], got["method"][o + i], got["pos_world"][o + i]) == [], (c.name, pos)
                others = np.arange(pb["n"]) != i
                assert (got["code"][o:o + pb["n"]][others] == dlc.filler(c)[1]).all(), (c.name, pos)
                seen += 1
            largest = max(largest, len(chunk))
    assert seen == 5 * len(dlc.pair_cases()) and largest == dlc.N_PROBLEMS          # no case is left out; a call of 32 problems occurs


def test_every_pair_as_one_problem_of_32(pair_ctx):
    for c in dlc.pair_cases():
        for pos in dlc.PROBLEM_POSITIONS:
            got = create(pair_ctx, c, dlc.problems_around(c, pos))
            o = int(got["offsets"][pos])
            assert got["offsets"][pos + 1] == o + 1
            assert dlc.pair_holds(c, got["code"][o], got["method"][o], got["pos_world"][o]) == [], (c.name, pos)


# ---- depths ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def depth_ctx(hip_lib):
    """the context, name -> slot of each picture (slot 0: the zero left picture), name -> its downloaded levels"""
    pictures = dlc.pictures()
    ctx = make_ctx(hip_lib, width=dlc.WIDTH, height=dlc.HEIGHT, levels=dlc.LEVELS, max_frames=1 + len(pictures), intrinsics=dlc.INTRINSICS)
    ctx.upload_gray(0, pictures["zero"])
    slots = {}
    for s, (name, img) in enumerate(pictures.items(), 1):
        ctx.upload_gray(s, img)
        slots[name] = s
    ctx.build_pyramid(0, 1 + len(pictures))
    levels = {name: [ctx.download_level(s, l) for l in range(dlc.LEVELS)] for name, s in slots.items()}
    assert np.array_equal(levels["level0"][0], pictures["level0"]) and not any(lv.any() for lv in levels["zero"])
    yield ctx, slots, levels
    ctx.close()


@pytest.mark.parametrize("row", dlc.DEPTH_ROWS)
def test_every_depth_case(depth_ctx, row):
    ctx, slots, levels = depth_ctx
    cases = [c for c in dlc.depth_cases() if c.row == row]
    assert cases
    for c in cases:
        want = sr.match(levels["zero"], levels[c.right], c.kl, c.kr, sr.params(**c.params), fx=dlc.FX)
        got = ctx.stereo_match(0, slots[c.right], c.kl, c.kr, **c.params)
        got.update(ctx.stereo_candidates(0, slots[c.right], c.kl, c.kr, **c.params))
        for k in sr.OUTPUTS + sr.STAGES:
            assert got[k].dtype == want[k].dtype and dlc.equal_bits(got[k], want[k]), (c.name, k)
        assert dlc.depth_holds(c, got) == [], c.name


def test_no_depth_case_is_left_out():
    """test_every_depth_case visits the rows of DEPTH_ROWS: every case belongs to one of them"""
    assert {c.row for c in dlc.depth_cases()} == set(dlc.DEPTH_ROWS) and len(dlc.depth_cases()) == 138 and len(dlc.pair_cases()) == 70
