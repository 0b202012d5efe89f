"""ctypes loader of tests/lms_ref.c, the restatement of the local-map selection (ygz_slam_amd/csrc/lms.hip) that
tests/test_lms_ref.py holds to a numpy / dict witness and tests/test_gpu_lms.py holds ygz_hip_local_map_select against.  Test
infrastructure: compiled with gcc into a temporary directory the first time it is used, never imported by the package.  Also the case
generator both tests share."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None

DEFAULTS = dict(max_keyframes=80, max_points=16384)
MAX_KEYFRAMES, MAX_COV, MAX_FRAMES, MAX_FRAME_ENTRIES, MAX_FEAT = 4096, 32, 1024, 32768, 32768
OUTPUTS = ("votes", "ref", "n_voters", "n_local", "local_kf", "n_pt", "n_cut", "local_pt", "fr_prior")


class Params(ctypes.Structure):
    """lr_params = ygz_lms_params"""
    _fields_ = [("max_keyframes", ctypes.c_int32), ("max_points", ctypes.c_int32)]


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="lms_ref_")
        so = os.path.join(d, "liblms_ref.so")
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "lms_ref.c")])
        _lib = ctypes.CDLL(so)
    return _lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def params(**kw):
    v = dict(DEFAULTS, **kw)
    return Params(int(v["max_keyframes"]), int(v["max_points"]))


def blank_outputs(case, fill=-7):
    """the nine output arrays of a case at their shapes, filled with a value no output can take"""
    K, F = case["K"], len(case["fr_off"]) - 1
    mp = int(dict(DEFAULTS, **case["params"])["max_points"])
    E = max(int(case["fr_off"][-1]), 1)
    shape = dict(votes=(F, K), ref=(F,), n_voters=(F,), n_local=(F,), local_kf=(F, K), n_pt=(F,), n_cut=(F,), local_pt=(F, mp), fr_prior=(E,))
    return {k: np.full(shape[k], fill, np.int32) for k in OUTPUTS}


def arrays(case):
    """the input arrays of a case in the ABI's types (kf, feat, cov and fr_pt of at least one element)"""
    one = lambda a: a if len(a) else np.zeros(1, np.int32)
    return dict(kf_bad=np.ascontiguousarray(case["kf_bad"], np.uint8), cov=one(np.ascontiguousarray(case["cov"], np.int32).reshape(-1)),
                off=np.ascontiguousarray(case["off"], np.int32), kf=one(np.ascontiguousarray(case["kf"], np.int32)),
                feat=one(np.ascontiguousarray(case["feat"], np.int32)),
                pt_bad=None if case["pt_bad"] is None else np.ascontiguousarray(case["pt_bad"], np.uint8),
                fr_off=np.ascontiguousarray(case["fr_off"], np.int32), fr_pt=one(np.ascontiguousarray(case["fr_pt"], np.int32)))


def select(case):
    """lr_select on a case: dict of the nine outputs (fr_prior cut to the frames' entries)"""
    a, o, q = arrays(case), blank_outputs(case), params(**case["params"])
    ip, bp = ctypes.c_int32, ctypes.c_uint8
    rc = lib().lr_select(case["K"], _p(a["kf_bad"], bp), case["C"], _p(a["cov"], ip), len(a["off"]) - 1, _p(a["off"], ip), _p(a["kf"], ip),
                         _p(a["feat"], ip), None if a["pt_bad"] is None else _p(a["pt_bad"], bp), len(a["fr_off"]) - 1, _p(a["fr_off"], ip),
                         _p(a["fr_pt"], ip), ctypes.byref(q), *[_p(o[k], ip) for k in OUTPUTS])
    assert rc == 0
    o["fr_prior"] = o["fr_prior"][:int(case["fr_off"][-1])]
    return o


# ---- cases: name -> dict(K, kf_bad [K], C, cov [K][C], off [P + 1], kf, feat [n_obs], pt_bad [P] or None, fr_off [F + 1], fr_pt, params {})

def _case(obs, K, frames, cov=None, kf_bad=(), pt_bad=None, **prm):
    """obs: per point a {keyframe: feature index}; frames: lists of points (-1: none); cov: K rows of equal length; kf_bad, pt_bad: indices"""
    lists = [sorted(o.items()) for o in obs]
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    kf = np.array([k for l in lists for k, _ in l], np.int32)
    feat = np.array([f for l in lists for _, f in l], np.int32)
    cov = np.zeros((K, 0), np.int32) if cov is None else np.asarray(cov, np.int32).reshape(K, -1)
    bad = np.zeros(K, np.uint8)
    bad[list(kf_bad)] = 1
    pb = None
    if pt_bad is not None:
        pb = np.zeros(len(obs), np.uint8)
        pb[list(pt_bad)] = 1
    fr_off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)
    fr_pt = np.array([p for f in frames for p in f], np.int32)
    assert len(obs) >= 1 and len(frames) >= 1 and (kf < K).all() and (cov < K).all() and (fr_pt < len(obs)).all()
    return dict(K=int(K), kf_bad=bad, C=int(cov.shape[1]), cov=cov, off=off, kf=kf, feat=feat, pt_bad=pb, fr_off=fr_off, fr_pt=fr_pt, params=prm)


def _random_map(rng, K, P, lo, hi, C=10, n_bad_kf=0, n_bad_pt=0, window=None):
    """P points with lo .. hi observers each out of a window of neighbouring keyframes; a keyframe's features are numbered in a random order
    with gaps, as the features of a keyframe that carry no point leave them; cov rows of C entries with some -1"""
    window = min(K, window or K)
    obs = []
    next_feat = [list(rng.permutation(2 * (P * hi // K + hi) + 8)) for _ in range(K)]
    for _ in range(P):
        first = int(rng.integers(0, K - window + 1))
        n = int(rng.integers(lo, min(hi, window) + 1))
        ks = rng.choice(np.arange(first, first + window), n, replace=False) if n else []
        obs.append({int(k): int(next_feat[int(k)].pop()) for k in ks})
    cov = np.full((K, C), -1, np.int32)
    for k in range(K):
        near = [c for c in range(max(0, k - 2 * C), min(K, k + 2 * C + 1)) if c != k]
        n = min(C, len(near))
        if n:
            cov[k, :n] = rng.choice(near, n, replace=False)
        cov[k, rng.uniform(size=C) < 0.1] = -1
    kf_bad = rng.choice(K, n_bad_kf, replace=False) if n_bad_kf else ()
    pt_bad = rng.choice(P, n_bad_pt, replace=False) if n_bad_pt else None
    return obs, cov, kf_bad, pt_bad


def _random_frame(rng, obs, n, around, spread, K):
    """n entries: points with an observer within `spread` of keyframe `around`, a fifth of the entries empty, a few points twice"""
    near = [p for p, o in enumerate(obs) if any(abs(k - around) <= spread for k in o)] or [0]
    f = [int(rng.choice(near)) if rng.uniform() > 0.2 else -1 for _ in range(n)]
    return f


# K = 4, C = 2; the numbers of HAND_OUT are worked out by hand
HAND = dict(obs=[{0: 0, 1: 2}, {1: 0}, {2: 1}, {0: 1, 3: 0}, {3: 1}], K=4, cov=[[1, 2], [0, 2], [3, -1], [2, 0]], frames=[[0, -1, 3], [2]])
HAND_OUT = dict(votes=[[2, 1, 0, 1], [0, 0, 1, 0]], ref=[0, 2], n_voters=[3, 1], n_local=[4, 2], local_kf=[[0, 1, 3, 2], [2, 3, -1, -1]],
                n_pt=[4, 3], n_cut=[1, 0], local_pt=[[0, 3, 1, 4], [2, 3, 4, -1]], fr_prior=[0, -1, 1, 0])


def _hand(**kw):
    return _case(HAND["obs"], HAND["K"], HAND["frames"], cov=HAND["cov"], **kw)


def _voters(n_voters, max_keyframes):
    """n_voters keyframes with one point each on the frame; voter i's covisibles are two keyframes nobody votes for"""
    K = n_voters + 2 * n_voters
    obs = [{k: 0} for k in range(n_voters)]
    cov = np.full((K, 2), -1, np.int32)
    for k in range(n_voters):
        cov[k] = [n_voters + 2 * k, n_voters + 2 * k + 1]
    return _case(obs, K, [list(range(n_voters))], cov=cov, max_keyframes=max_keyframes)


def cases():
    rng = np.random.default_rng(3407)
    c = {}
    c["hand"] = _hand(max_points=4)
    # frame 0 has entries and no point, frame 1 has no entry at all, frame 2 is an ordinary one
    c["frame_without_points"] = _case(HAND["obs"], 4, [[-1, -1, -1], [], [1, 4]], cov=HAND["cov"])
    c["point_twice"] = _case(HAND["obs"], 4, [[0, 3, 0], [4, 4, 4, 1]], cov=HAND["cov"])
    c["bad_point_on_frame"] = _case(HAND["obs"], 4, [[0, 3, 1], [3]], cov=HAND["cov"], pt_bad=[3])
    # keyframe 0 has the most votes and is bad: it is ref and not in the list (and its neighbours are not searched for it)
    c["bad_keyframe_most_votes"] = _case(HAND["obs"], 4, [[0, 3, 1]], cov=HAND["cov"], kf_bad=[0])
    c["vote_tie"] = _case([{1: 0, 2: 0}, {1: 1, 2: 1}, {0: 0}], 3, [[2, 0, 1], [0]], cov=[[1], [2], [0]])
    for n in (5, 6, 7):                                     # max_keyframes - 1 / = / + 1 voters: one extension step, none, none
        c["voters%d_max6" % n] = _voters(n, 6)
    c["voters3_max1"] = _voters(3, 1)
    # voters 0 and 1 both have keyframe 2 first: 0 takes it, 1 takes its next one, 3
    c["same_first_covisible"] = _case([{0: 0}, {1: 0}, {2: 0}, {3: 0}], 5, [[0, 1]], cov=[[2, 4], [2, 3], [-1, -1], [-1, -1], [-1, -1]])
    c["covisible_row_of_none"] = _case([{0: 0}, {1: 0}, {2: 0}], 3, [[0, 1]], cov=[[-1, -1, -1], [-1, 2, -1], [0, 1, -1]])
    c["bad_first_covisible"] = _case([{0: 0}, {1: 0}, {2: 0}, {3: 0}], 4, [[0]], cov=[[2, 3], [0, 0], [0, 0], [0, 0]], kf_bad=[2])
    c["covisible_is_a_voter"] = _case([{0: 0}, {1: 0}, {2: 0}], 3, [[0, 1]], cov=[[1, 2], [0, -1], [0, 1]])
    c["no_covisibles"] = _case(HAND["obs"], 4, HAND["frames"])
    # point 0 is seen by keyframes 1 (feature 9) and 3 (feature 2), both local: it stands at keyframe 1's rank with feature 9, behind point 1
    c["point_of_two_local_keyframes"] = _case([{1: 9, 3: 2}, {1: 4}, {3: 0}, {3: 5}], 4, [[1, 2]], cov=[[-1], [-1], [-1], [-1]])
    # point 2's only observer is bad, so outside the list: it votes, it is ref's point, and its prior is -1
    c["observers_outside_the_list"] = _case([{0: 0}, {0: 1, 1: 0}, {2: 0}], 3, [[2, 2, 0]], cov=[[1], [0], [0]], kf_bad=[2])
    for mp in (4, 5, 6):                                    # frame 0 of the hand-made map has 5 local points
        c["max_points%d_of5" % mp] = _hand(max_points=mp)
    c["max_points1"] = _hand(max_points=1)
    c["shared_feature"] = _case([{0: 3}, {0: 1, 1: 1}, {0: 1}, {0: 0, 1: 1}], 2, [[0], [1, -1]], cov=[[1], [0]])
    for n in (63, 64, 65, 255, 256):                        # point 0 is seen by n keyframes
        obs, cov, _, _ = _random_map(rng, n + 3, 40, 1, 5)
        obs[0] = {k: int(rng.integers(0, MAX_FEAT)) for k in range(n)}
        c["list_of_%d" % n] = _case(obs, n + 3, [[0, 5, -1, 7], [3, 9]], cov=cov, max_keyframes=n // 2 if n % 2 else 4096)
    for n in (255, 256, 257):                               # keyframe 1 sees n points
        obs, cov, _, _ = _random_map(rng, 6, n + 20, 0, 3)
        feats = rng.permutation(2 * n)
        for p in range(n):
            obs[p][1] = int(feats[p])
        c["keyframe_of_%d" % n] = _case(obs, 6, [[0, 1, 2], [n + 3, n + 5, -1]], cov=cov, max_points=n - 1 if n == 256 else 16384)
    c["k1"] = _case([{0: 4}, {}, {0: 2}], 1, [[0], [1], [-1, 2, 2]], cov=[[-1]])
    c["k1_bad"] = _case([{0: 4}, {}, {0: 2}], 1, [[0], [1]], kf_bad=[0])
    c["k2"] = _case([{0: 1, 1: 0}, {1: 1}, {0: 0}, {}], 2, [[1], [2], [3, 0]], cov=[[1], [0]])
    obs, cov, kb, pb = _random_map(rng, 130, 2500, 1, 9, n_bad_kf=9, n_bad_pt=60, window=30)
    for F in (1, 3, 65):
        frames = [_random_frame(rng, obs, int(rng.integers(1, 300)), int(rng.integers(0, 130)), 4, 130) for _ in range(F)]
        c["k130_frames%d" % F] = _case(obs, 130, frames, cov=cov, kf_bad=kb, pt_bad=pb, max_keyframes=20 if F == 3 else 80,
                                       max_points=1300 if F == 65 else 16384)
    obs, cov, kb, pb = _random_map(rng, 4096, 6000, 1, 6, C=32, n_bad_kf=200, n_bad_pt=100, window=300)
    frames = [_random_frame(rng, obs, 400, a, 120, 4096) for a in (100, 2000, 4000)] + [list(range(0, 6000, 3))]
    c["k4096"] = _case(obs, 4096, frames, cov=cov, kf_bad=kb, pt_bad=pb, max_keyframes=4096, max_points=3000)
    c["k4096_max80"] = _case(obs, 4096, frames[:2], cov=cov, kf_bad=kb, pt_bad=pb)
    return c


def smaller_case():
    """a second problem, smaller in every array than most of the cases: what a context's scratch holds from the call before must not matter"""
    return _case(HAND["obs"], 4, [[4, 1]], cov=HAND["cov"], max_keyframes=3, max_points=2)
