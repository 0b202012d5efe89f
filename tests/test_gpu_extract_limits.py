"""The extractor kernels (ygz_slam_amd/csrc/detect.hip: k_fast_select, k_compact, k_describe<1>, k_describe<8>) on the crafted cases of
tests/extract_cases.py and over a sweep of configurations, against the cases' literals and the oracle.  tests/test_extract_cases.py shows on
the CPU that the cases separate every wrong variant of every rule of DESIGN.md section 38 and that no configuration of the sweep is vacuous.
Every comparison is an equality: positions, levels, score bits, angles and descriptors (test_gpu_parity._kp_check's rules), and the score and
NMS maps where debug_maps is on."""
import functools

import numpy as np
import pytest
from conftest import make_ctx
from ygz_slam_amd import synth

import extract_cases as ec
from test_extract_cases import as_tuples, oracle_maps, oracle_params
from test_gpu_parity import _kp_check

pytestmark = pytest.mark.gpu

# (picture, size, fast_threshold, cell_size, levels, nms_tie_suppress): a covering subset of {texture, noise} x {208 x 136, 206 x 135, 640 x 480} x
# {0, 7, 15, 40} x {1, 3, 4, 10, 16, 64} x {1, 2, 3, 5} x {0, 1}: every value of every parameter, both unit sizes with every threshold they
# may have, threshold 0 on the noise picture only, and one 640 x 480 frame under two configurations: three levels at cell 4 (levels 1 and 2
# have interior tiles there and win cells), and cell 64 on level 0 alone (208 x 136 has only 12 cells of 64, fewer than the 50 keypoints
# asked of a unit-size configuration, and in a cell of 64 pixels level 0 always holds the strongest corner, so no other level could be asked
# to win one).  tests/test_extract_cases.py::test_the_sweep_cannot_pass_vacuously holds the list to that.
SWEEP = [
    ("noise", ec.UNIT, 0, 10, 3, 0),
    ("noise", ec.TWIN, 0, 3, 2, 1),
    ("noise", ec.UNIT, 15, 16, 1, 1),
    ("texture", ec.UNIT, 7, 1, 3, 0),
    ("texture", ec.UNIT, 15, 3, 2, 1),
    ("texture", ec.UNIT, 40, 4, 1, 0),
    ("texture", ec.UNIT, 7, 16, 5, 1),
    ("texture", ec.TWIN, 15, 10, 3, 1),
    ("texture", ec.TWIN, 40, 1, 5, 0),
    ("texture", ec.TWIN, 7, 4, 2, 0),
    ("texture", (640, 480), 15, 4, 3, 0),
    ("texture", (640, 480), 15, 64, 1, 1),
]


@functools.lru_cache(maxsize=None)
def sweep_picture(pic, size, seed=3):
    w, h = size
    if pic == "noise":
        return np.random.default_rng(seed * 1000 + w).integers(0, 256, (h, w), dtype=np.uint8)
    tex, m = synth.make_texture(seed, w, h, margin=max(80, w // 4))
    return synth.render(tex, m, [0, 0, 0, 1, 0, 0, 0], w, h, 1.0, seed * 1000)[0]


def ctx_for(hip_lib, size, params, max_frames=1, debug_maps=None):
    return make_ctx(hip_lib, width=size[0], height=size[1], levels=params["levels"], max_frames=max_frames,
                    debug_maps=params["debug_maps"] if debug_maps is None else debug_maps, fast_threshold=params["fast_threshold"],
                    cell_size=params["cell_size"], nms_tie_suppress=params["nms_tie_suppress"])


def key_of(c):
    return (c.picture.shape[::-1],) + tuple(sorted(c.params.items()))


def got_tuples(kp):
    return [(float(p[0]), float(p[1]), int(l), int(s)) for p, l, s in zip(kp["px"], kp["level"], kp["score"].view(np.uint32))]


class Contexts:
    """one context per (size, parameters, slots) for the cases of a row"""
    def __init__(self, hip_lib):
        self.lib, self.ctx = hip_lib, {}

    def get(self, c, max_frames=1):
        k = key_of(c) + (max_frames,)
        fresh = k not in self.ctx
        if fresh:
            self.ctx[k] = ctx_for(self.lib, c.picture.shape[::-1], c.params, max_frames)
        return self.ctx[k], fresh

    def close(self):
        for x in self.ctx.values():
            x.close()


@functools.lru_cache(maxsize=None)
def _oracle_of(oracle, name):
    c = next(c for c in ec.cases() if c.name == name)
    lv = oracle.pyramid(c.picture, c.params["levels"])
    return lv, oracle.detect(lv, oracle_params(oracle, c), c.occupied)


@pytest.mark.parametrize("row", ec.ROWS)
def test_every_case_alone(hip_lib, oracle, row):
    """each case in a context of one slot: the literals, the oracle, and the maps where debug_maps is on.  Row "level 3" is the 1408 x 1408
    picture of four levels"""
    pool = Contexts(hip_lib)
    for c in (c for c in ec.cases() if c.row == row):
        ctx, _ = pool.get(c)
        ctx.upload_gray(0, c.picture)
        ctx.build_pyramid(0, 1)
        ctx.detect(0, 1, occupied=None if c.occupied is None else c.occupied[None])
        kp = ctx.get_keypoints(0)
        lv, ok_ = _oracle_of(oracle, c.name)
        maps = [ctx.get_fast_maps(0, L) for L in range(len(lv))] if c.params["debug_maps"] else None
        assert ec.holds(c, got_tuples(kp), None if maps is None else [m[0] for m in maps], None if maps is None else [m[1] for m in maps]) == [], c.name
        _kp_check(kp, ok_)
        assert ctx.keypoint_count(0) == len(c.expected["keypoints"]), c.name
        if maps is not None:
            for L, im in enumerate(lv):
                smap, nmap = oracle_maps(oracle, im, c.params["fast_threshold"], c.params["nms_tie_suppress"])
                assert np.array_equal(maps[L][0], smap) and np.array_equal(maps[L][1], nmap), (c.name, L)
    pool.close()


@pytest.mark.parametrize("row", ec.ROWS)
def test_every_case_embedded(hip_lib, oracle, row):
    """the case in slots 3 and 16 of detect(0, 17) (k_describe<8>, the surplus slices of the XCD remap: 24 launched for 17) and as the only
    slot of detect(5, 1) in a context of 24 slots; the other slots hold the filler, give the filler's literals, and the slots outside a call
    keep the keypoints they had.  A case's mask goes to its own slots, the others get an empty one"""
    pool = Contexts(hip_lib)
    for c in (c for c in ec.cases() if c.row == row):
        size = c.picture.shape[::-1]
        lv, ok_ = _oracle_of(oracle, c.name)
        fill = ec.filler(size)
        f_lit = ec.filler_keypoints(c.params)
        prm_f = oracle_params(oracle, c)
        f_ok = oracle.detect(oracle.pyramid(fill, c.params["levels"]), prm_f)
        assert as_tuples(f_ok) == f_lit, c.name

        def is_case(kp):
            assert ec.holds(c, got_tuples(kp)) == [], c.name
            _kp_check(kp, ok_)

        def is_filler(kp):
            assert got_tuples(kp) == f_lit, c.name
            _kp_check(kp, f_ok)
        # ---- 17 slots in one call
        ctx, fresh = pool.get(c, 17)
        if fresh:
            ctx.upload_gray_batch(0, np.stack([fill] * 17))
        for s in (3, 16):
            ctx.upload_gray(s, c.picture)
        ctx.build_pyramid(0, 17)
        occ = None
        if c.occupied is not None:
            occ = np.zeros((17, len(c.occupied)), np.uint8)
            occ[3] = occ[16] = c.occupied
        ctx.detect(0, 17, occupied=occ)
        for s in range(17):
            (is_case if s in (3, 16) else is_filler)(ctx.get_keypoints(s))
        # ---- one slot in the middle of 24
        ctx, fresh = pool.get(c, 24)
        if fresh:
            ctx.upload_gray_batch(0, np.stack([fill] * 24))
            ctx.build_pyramid(0, 24)
            ctx.detect(0, 24)
        ctx.upload_gray(5, c.picture)
        ctx.build_pyramid(5, 1)
        ctx.detect(5, 1, occupied=None if c.occupied is None else c.occupied[None])
        is_case(ctx.get_keypoints(5))
        for s in (0, 4, 6, 23):
            is_filler(ctx.get_keypoints(s))
    pool.close()


@pytest.mark.parametrize("cfg", SWEEP, ids=lambda c: "%s-%dx%d-thr%d-cell%d-levels%d-tie%d" % ((c[0],) + c[1] + c[2:]))
def test_configuration_sweep(hip_lib, oracle, cfg):
    pic, size, thr, cell, levels, tie = cfg
    img = sweep_picture(pic, size)
    params = dict(levels=levels, fast_threshold=thr, cell_size=cell, nms_tie_suppress=tie, debug_maps=True)
    ctx = ctx_for(hip_lib, size, params)
    ctx.upload_gray(0, img)
    ctx.build_pyramid(0, 1)
    ctx.detect(0, 1)
    p = oracle.default_params(size[0], size[1], levels)
    p.cell_size, p.detection_threshold, p.nms_tie_suppress = cell, float(thr), tie
    lv = oracle.pyramid(img, levels)
    _kp_check(ctx.get_keypoints(0), oracle.detect(lv, p))
    for L in range(levels):
        smap, nmap = oracle_maps(oracle, lv[L], thr, tie)
        gs, gn = ctx.get_fast_maps(0, L)
        assert np.array_equal(gs, smap) and np.array_equal(gn, nmap), L
    ctx.close()
    # tiles outside InFrame(20, L) are skipped only without the maps: the keypoints are the same
    ctx = ctx_for(hip_lib, size, params, debug_maps=False)
    ctx.upload_gray(0, img)
    ctx.build_pyramid(0, 1)
    ctx.detect(0, 1)
    _kp_check(ctx.get_keypoints(0), oracle.detect(lv, p))
    ctx.close()


def _seventeen():
    """15 noise pictures, a flat one (no keypoint) and a crafted one (11 keypoints) at 208 x 136"""
    pics = [sweep_picture("noise", ec.UNIT, seed) for seed in range(10, 25)]
    pics.insert(6, ec.flat(ec.UNIT))
    pics.append(next(c.picture for c in ec.cases() if c.name.endswith("the count: cell 10")))
    return pics


def test_both_describe_instantiations(hip_lib, oracle):
    """k_describe<8> (17 slots in one call) and k_describe<1> (17 calls of one slot) on the same pictures: equal to the oracle and to each other"""
    pics = _seventeen()
    ks = [oracle.detect(oracle.pyramid(im, 2), oracle.default_params(ec.UNIT[0], ec.UNIT[1], 2)) for im in pics]
    counts = [len(k) for k in ks]
    assert counts[6] == 0 and counts[16] == 11 and any(n % 32 for n in counts) and max(counts) > 64
    ctx = make_ctx(hip_lib, width=ec.UNIT[0], height=ec.UNIT[1], levels=2, max_frames=17)
    ctx.upload_gray_batch(0, np.stack(pics))
    ctx.build_pyramid(0, 17)
    ctx.detect(0, 17)
    batch = [ctx.get_keypoints(s) for s in range(17)]
    for s in range(17):
        _kp_check(batch[s], ks[s])
    for s in range(17):
        ctx.detect(s, 1)
    for s in range(17):
        one = ctx.get_keypoints(s)
        _kp_check(one, ks[s])
        assert all(one[f].tobytes() == batch[s][f].tobytes() for f in ("px", "level", "score", "angle", "desc")), s
    ctx.close()


@pytest.mark.parametrize("cell", [3, 10])
def test_random_occupied_masks(hip_lib, oracle, cell):
    """nine slots, a different mask of density 0.5 in each: cell 10 keeps the flags of a tile in LDS at every level, cell 3 reads them from
    global memory at levels 1 and 2 (occ_fits)"""
    pics = _seventeen()[:9]
    w, h = ec.UNIT
    p = oracle.default_params(w, h, 3)
    p.cell_size = cell
    cols, rows = ec.grid(ec.UNIT, cell)
    occ = (np.random.default_rng(cell).random((9, cols * rows)) < 0.5).astype(np.uint8)
    ctx = make_ctx(hip_lib, width=w, height=h, levels=3, max_frames=9, cell_size=cell)
    assert ctx.cells == cols * rows
    ctx.upload_gray_batch(0, np.stack(pics))
    ctx.build_pyramid(0, 9)
    ctx.detect(0, 9, occupied=occ)
    levels_seen = set()
    for s in range(9):
        ok_ = oracle.detect(oracle.pyramid(pics[s], 3), p, occ[s])
        free = oracle.detect(oracle.pyramid(pics[s], 3), p)
        assert s == 6 or 0 < len(ok_) < len(free)
        levels_seen |= set(ok_["level"].tolist())
        _kp_check(ctx.get_keypoints(s), ok_)
    assert levels_seen == {0, 1}
    ctx.close()
