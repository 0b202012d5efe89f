"""The scenes of the stereo bundle adjustment's tests, shared by tests/test_sba_ref.py (the restatement against its witnesses) and
tests/test_gpu_sba.py (the device against the restatement): name -> (make, parameters).  Every scene is a valid call of ygz_hip_stereo_ba."""
import numpy as np

import gba_ref as gb
import sba_ref as sb


def _behind():
    """a point half a camera distance behind one of its cameras: FAILED in round 0"""
    g = sb.scene(3, 12, 2, seed=24)
    v = g["edge_pose"][np.flatnonzero(g["edge_point"] == 5)[0]]
    g["points"][5] = 1.5 * (-gb.rotation(g["poses"][v][:4]).T @ g["poses"][v][4:])
    return g


def _displace(g, edges, seed, times=1.0):
    rng = np.random.default_rng(seed)
    for e in edges:
        a, m = rng.uniform(0, 2 * np.pi), times * rng.uniform(20, 60) * 2.0 ** g["level"][e]
        g["obs"][e] += [m * np.cos(a), m * np.sin(a), m * np.cos(a)]
        g["displaced"][e] = True
    return g


def _one_edge_left():
    """points of two observations; the first observation of points 0, 7 and 14 is displaced: each of them enters round 1 with one active edge"""
    g = sb.scene(4, 24, 2, seed=41)
    return _displace(g, [int(np.flatnonzero(g["edge_point"] == l)[0]) for l in (0, 7, 14)], 42)


def _pose_without_edges():
    """every observation of free pose 3 is displaced by 100 to 300 pixels of its level, each in its own direction: pose 3 enters round 1
    without an active edge"""
    g = sb.scene(6, 60, 4, seed=43)
    return _displace(g, np.flatnonzero(g["edge_pose"] == 3), 44, times=5.0)


def _nothing_left():
    """two poses, eight points, every observation hundreds of pixels off: one LM iteration leaves no inlier, and round 1 has no active edge"""
    g = sb.scene(2, 8, 2, seed=45, noise=0.0)
    g["obs"] += np.random.default_rng(46).normal(0, 300, g["obs"].shape) * (2.0 ** g["level"])[:, None]
    return g


def _absent():
    """every fifth edge absent (points keep three or four present edges), the absent ones with a non-finite observation that is never read"""
    g = sb.scene(8, 80, 4, outliers=0.1, seed=47, fixed=(0, 4))
    g["kind"][::5] = 0
    g["obs"][::5] = np.nan
    return g


# (d): sized as the global bundle adjustment's scenes, levels cycling 0 .. 3, noise 0.5 x 2^level on all three coordinates, outliers displaced
# by 20 to 60 pixels of the edge's level.  The relative-decrease stop is switched on at 1e-6, as for the pose optimisation's scenes: with
# the default 1e-9 a round may end at the rounding floor of its cost, where a witness that adds in another order cannot follow the last
# accept / reject decision
D_PARAMS = dict(min_rel_decrease=1e-6)
SCENES_D = {
    "half_5x40": (lambda: sb.scene(5, 40, 3, seed=21), D_PARAMS),
    "half_8x80_outliers": (lambda: sb.scene(8, 80, 4, outliers=0.1, seed=21, fixed=(0, 4)), D_PARAMS),
    "stereo_6x60_outliers": (lambda: sb.scene(6, 60, 3, stereo="all", outliers=0.1, seed=29, fixed=(0, 3)), D_PARAMS),
    "mono_12x100_outliers": (lambda: sb.scene(12, 100, 4, stereo="none", outliers=0.1, seed=34), D_PARAMS),
}

# (f): the branches, by name
SCENES_F = {
    "flags_change_between_rounds": (lambda: sb.scene(8, 80, 4, outliers=0.1, seed=24, fixed=(0, 4)), {}),
    "failed_in_round_0": (_behind, {}),
    "point_left_with_one_active_edge": (_one_edge_left, {}),
    "free_pose_left_without_an_edge": (_pose_without_edges, {}),
    "round_with_no_active_edge": (_nothing_left, dict(iterations=(1, 3))),
    "kind_0_among_the_edges": (_absent, {}),
    "repeated_edge": (lambda: sb.scene(4, 30, 3, seed=25, repeat_edge=True), {}),
    "two_fixed_poses": (lambda: sb.scene(6, 60, 3, seed=27, fixed=(1, 4)), {}),
    "rounds_1": (lambda: sb.scene(5, 40, 3, outliers=0.1, seed=28), dict(rounds=1, iterations=(7,))),
    "rounds_4": (lambda: sb.scene(5, 40, 3, outliers=0.1, seed=28), dict(rounds=4, robust_rounds=2, iterations=(3, 4, 5, 6))),
    "robust_rounds_0": (lambda: sb.scene(5, 40, 3, outliers=0.1, seed=29), dict(robust_rounds=0)),
    "robust_rounds_4": (lambda: sb.scene(5, 40, 3, outliers=0.1, seed=29), dict(rounds=4, robust_rounds=4, iterations=(4, 4, 4, 4))),
    "rejected_trial": (lambda: sb.scene(4, 30, 3, seed=25), dict(rounds=1, iterations=(30,), min_rel_decrease=0.0)),
    "capped_cg": (lambda: sb.scene(12, 100, 4, seed=26), dict(cg_max_iterations=3)),
}


_EDGE_KEYS = ("edge_pose", "edge_point", "obs", "kind", "level", "displaced")


def _pose_degree(deg):
    """four poses, the free pose 1 with exactly `deg` edges: every point is seen by poses 0, 2 and 3 and the first `deg` also by pose 1"""
    g = sb.scene(4, deg + 5, 4, seed=50 + deg)                         # all four poses see every point, edges sorted by point
    keep = ~((g["edge_pose"] == 1) & (g["edge_point"] >= deg))
    for k in _EDGE_KEYS:
        g[k] = g[k][keep]
    return g


def _edges(E):
    """exactly E edges: ceil(E / 4) points seen by four poses each; the last point loses up to two edges, the one before it the third"""
    L = (E + 3) // 4
    g = sb.scene(4, L, 4, seed=60 + E % 7)
    drop = 4 * L - E
    keep = np.ones(4 * L, bool)
    keep[4 * L - min(drop, 2):] = False
    if drop == 3:
        keep[4 * L - 5] = False
    for k in _EDGE_KEYS:
        g[k] = g[k][keep]
    assert len(g["edge_pose"]) == E
    return g


# sizes at which the kernels take another path: the chunk edge of the edge kernels, the workgroup edge of the point kernels, the lane stride
# of the pose kernels, and the smallest problem
SCENES_SIZE = {
    "e1023": (lambda: _edges(1023), {}), "e1024": (lambda: _edges(1024), {}), "e1025": (lambda: _edges(1025), {}),
    "l255": (lambda: sb.scene(4, 255, 3, seed=71), {}), "l256": (lambda: sb.scene(4, 256, 3, seed=72), {}), "l257": (lambda: sb.scene(4, 257, 3, seed=73), {}),
    "deg255": (lambda: _pose_degree(255), {}), "deg256": (lambda: _pose_degree(256), {}), "deg257": (lambda: _pose_degree(257), {}),
    "p2_l8": (lambda: sb.scene(2, 8, 2, seed=31), {}),
}
