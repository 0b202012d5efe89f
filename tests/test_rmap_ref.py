"""tests/rmap_ref.py, the host specification of the resident local-map call: its filter (steps 2 to 4 of the header)
is held to a numpy witness (boolean mask and cumulative sum) on random lists and to literal cases worked out by hand, and the whole
composition runs on a small fabricated scene.  No device."""
import numpy as np
import pytest

import popt_ref
import proj_ref
import rmap_ref as rr

K4 = popt_ref.DEFAULT_K
W, H, Z = 320, 240, 4.0


def witness(local_pt, n_pt, ref):
    """the filter by mask and cumulative sum"""
    F, MP = local_pt.shape
    out, n_out, moved = np.full((F, MP), -1, np.int32), np.zeros(F, np.int32), []
    for f in range(F):
        row = local_pt[f, :n_pt[f]]
        keep = ref[row] == 0
        pos = np.cumsum(keep) - 1
        moved.append(np.where(keep, pos, -1).astype(np.int32))
        out[f, :keep.sum()] = row[keep]
        n_out[f] = keep.sum()
    return out, n_out, n_pt - n_out, moved


@pytest.mark.parametrize("seed", range(6))
def test_filter_equals_the_mask_and_cumsum_witness(seed):
    rng = np.random.default_rng(seed)
    P, F, MP = 900, 5, 600
    ref = (rng.uniform(size=P) < (0.0, 0.1, 0.5, 0.9, 1.0, 0.3)[seed]).astype(np.uint8)
    n_pt = np.array([0, 1, 255, 257, 600], np.int32)
    local_pt = np.full((F, MP), -1, np.int32)
    for f in range(F):
        local_pt[f, :n_pt[f]] = rng.integers(0, P, n_pt[f])               # a point may stand twice
    got, want = rr.filter_lists(local_pt, n_pt, ref), witness(local_pt, n_pt, ref)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(g, w)
    assert all(np.array_equal(g, w) for g, w in zip(got[3], want[3]))
    cells = 700
    fr_off = np.array([0, 10, 10, 300, 650, 1350], np.int32)
    fr_prior = np.concatenate([rng.integers(-1, max(int(n), 1), int(b - a)) if n else np.full(b - a, -1) for n, a, b in
                               zip(n_pt, fr_off[:-1], fr_off[1:])]).astype(np.int32)
    prior = rr.prior_rows(fr_off, fr_prior, got[3], cells)
    for f in range(F):
        at = fr_prior[fr_off[f]:fr_off[f + 1]]
        w = np.where(at >= 0, want[3][f][np.maximum(at, 0)] if n_pt[f] else -1, -1)
        assert np.array_equal(prior[f, :len(at)], w) and (prior[f, len(at):] == -1).all()


def test_filter_literal_cases():
    state = np.array([1, 0, 1, 2, 1, 1], np.int32)
    has = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    ref = rr.refused(state, has)
    assert ref.tolist() == [0, 1, 1, 1, 0, 0] and rr.refused(state, None).tolist() == [0, 1, 0, 1, 0, 0]
    local_pt = np.array([[1, 0, 4, 4, 3, 5, -1], [1, 2, 3, -1, -1, -1, -1], [5, 4, 0, -1, -1, -1, -1], [-1] * 7], np.int32)
    lp, n, rem, moved = rr.filter_lists(local_pt, np.array([6, 3, 3, 0], np.int32), ref)
    assert lp.tolist() == [[0, 4, 4, 5, -1, -1, -1], [-1] * 7, [5, 4, 0, -1, -1, -1, -1], [-1] * 7]
    assert n.tolist() == [4, 0, 3, 0] and rem.tolist() == [2, 3, 0, 0]
    assert [m.tolist() for m in moved] == [[-1, 0, 1, 2, -1, 3], [-1, -1, -1], [0, 1, 2], []]
    # the prior: an entry on a refused point, on a kept one, without a position, past the frame's entries
    fr_off = np.array([0, 4, 6, 6, 7], np.int32)
    fr_prior = np.array([0, 5, -1, 2, 1, -1, -1], np.int32)
    assert rr.prior_rows(fr_off, fr_prior, moved, 5).tolist() == [[-1, 3, -1, 1, -1], [-1, -1, -1, -1, -1], [-1] * 5, [-1] * 5]
    with pytest.raises(AssertionError):
        rr.prior_rows(fr_off, fr_prior, moved, 3)                         # a frame with more entries than cells


def test_strided_layout_leaves_the_tail_alone():
    o = dict(match=np.arange(5, dtype=np.int32), proj=np.arange(15, dtype=np.float64).reshape(5, 3), status=np.zeros(3, np.int32),
             offsets=np.array([0, 2, 2, 5]))
    for k in rr.PER_POINT:
        o.setdefault(k, np.arange(5, dtype=np.int32))
    s = rr.strided(o, np.array([2, 0, 3]), 4)
    assert s["match"].tolist() == [[0, 1, -7, -7], [-7] * 4, [2, 3, 4, -7]] and s["proj"].shape == (3, 4, 3) and s["proj"][2, 2, 2] == 14.0
    assert "offsets" not in s and s["status"] is o["status"]


def scene(n_kp=120, n_pt=150, seed=1):
    """a frame of lattice keypoints at depth Z and a world of points on them"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(20, W - 20, 22.0), np.arange(20, H - 20, 22.0))
    px = np.stack([gx.reshape(-1), gy.reshape(-1)], 1)[:n_kp] + rng.uniform(-3, 3, (n_kp, 2))
    fr = dict(px=px, level=rng.integers(0, 3, n_kp).astype(np.int32), desc=rng.integers(0, 256, (n_kp, 32)).astype(np.uint8),
              depth=np.full(n_kp, Z), has_mp=(rng.uniform(size=n_kp) < 0.6).astype(np.uint8))
    j = np.arange(n_pt) % n_kp
    p = px[j] + rng.uniform(-0.7, 0.7, (n_pt, 2)) * (np.arange(n_pt) >= n_kp)[:, None]
    pw = np.stack([(p[:, 0] - K4[2]) / K4[0] * Z, (p[:, 1] - K4[3]) / K4[1] * Z, np.full(n_pt, Z)], 1)
    desc = np.stack([proj_ref.flip_bits(rng, fr["desc"][jj], int(rng.integers(0, 21))) for jj in j])
    return fr, rr.make_world(pw, desc, fr["level"][j], 4, seed + 1), j


def test_composition_on_a_fabricated_scene():
    fr, world, j = scene()
    rr.refuse(world, [0, 7, 20, 149])
    n_kp = len(fr["level"])
    fr_pt = np.full(n_kp, -1, np.int32)
    fr_pt[:40:2] = np.arange(0, 40, 2)                                    # keypoint k already holds point k: a vote and a prior
    T = [[0, 0, 0, 1.0, 0.3 * Z / K4[0], 0, 0]]
    o = rr.resident(world, {0: fr}, [0], T, [0, n_kp], fr_pt, cells=192, lms=dict(max_points=140), K=K4, w=W, h=H, L=3)
    assert o["n_pt"][0] + o["n_removed"][0] + o["n_cut"][0] == 150 and o["n_removed"][0] >= 3 and o["n_cut"][0] == 10
    assert o["match"].shape == (1, 140) and (o["match"][0, o["n_pt"][0]:] == rr.FILL).all()
    # keypoint 0's point was refused: no prior; keypoint 2's was kept
    assert o["prior"][0, 0] == -1 and o["prior"][0, 2] >= 0 and o["local_pt"][0, o["prior"][0, 2]] == 2
    assert o["counts"][0, 2] == (o["prior"][0] >= 0).sum() and o["counts"][0, 3] == o["n_pt"][0]
    assert o["counts"][0, 6] > 30 and o["status"][0] == 0, o["counts"]   # the scene is about something
