"""ctypes loader of libygz_hip.so (the C ABI declared in include/ygz_hip.h).

This is harness plumbing for tests/ and bench.py: numpy arrays in, numpy arrays out, every
call goes straight through the C ABI.  There is NO fallback path: if the HIP library is
missing or no gfx950 device is usable the calls raise.
"""
import ctypes as C
import os
import sys
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libygz_hip.so")
MAX_LEVELS = 8

OK, E_INVALID, E_HIP, E_NO_DEVICE, E_CAPACITY, E_STATE = 0, -1, -2, -3, -4, -5
ABI_VERSION = 6                     # YGZ_HIP_ABI_VERSION of include/ygz_hip.h this file mirrors


class YgzHipError(RuntimeError):
    def __init__(self, code, what, hip_err=0):
        super().__init__("%s failed: code %d (hip error %d)" % (what, code, hip_err))
        self.code = code


class Params(C.Structure):
    _fields_ = [("image_width", C.c_int), ("image_height", C.c_int), ("pyramid_levels", C.c_int),
                ("cell_size", C.c_int), ("fast_threshold", C.c_int), ("nms_tie_suppress", C.c_int),
                ("max_frames", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("debug_maps", C.c_int)]


class KptSoa(C.Structure):
    _fields_ = [("px", C.POINTER(C.c_double)), ("level", C.POINTER(C.c_int32)), ("score", C.POINTER(C.c_float)),
                ("angle", C.POINTER(C.c_float)), ("desc", C.POINTER(C.c_uint8))]


class AlignPair(C.Structure):
    _fields_ = [("ref_slot", C.c_int), ("cur_slot", C.c_int), ("T_ref", C.c_double * 7), ("T_cur", C.c_double * 7)]


class LocalMap(C.Structure):
    _fields_ = [("n_points", C.c_int), ("pos_world", C.POINTER(C.c_double)), ("point_bad", C.POINTER(C.c_uint8)),
                ("n_keyframes", C.c_int), ("kf_slot", C.POINTER(C.c_int32)), ("kf_T", C.POINTER(C.c_double)),
                ("n_candidates", C.c_int), ("cand_point", C.POINTER(C.c_int32)), ("cand_kf", C.POINTER(C.c_int32)),
                ("cand_level", C.POINTER(C.c_int32)), ("cand_px_ref", C.POINTER(C.c_double))]


class KltParams(C.Structure):
    _fields_ = [("win", C.c_int), ("max_level", C.c_int), ("max_iter", C.c_int), ("eps", C.c_double),
                ("min_eig_threshold", C.c_double), ("use_initial_flow", C.c_int)]


class BaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int), ("n_points", C.c_int), ("n_edges", C.c_int),
                ("poses", C.POINTER(C.c_double)), ("pose_fixed", C.POINTER(C.c_uint8)),
                ("points", C.POINTER(C.c_double)), ("edge_pose", C.POINTER(C.c_int32)),
                ("edge_point", C.POINTER(C.c_int32)), ("obs", C.POINTER(C.c_double)),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("huber_delta", C.c_double), ("formulation", C.c_int),
                ("point_fixed", C.POINTER(C.c_uint8)), ("edge_huber", C.POINTER(C.c_double)),
                ("edge_enable", C.POINTER(C.c_uint8))]


class CeresOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int), ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("jacobi_scaling", C.c_int), ("max_num_consecutive_invalid_steps", C.c_int), ("fail_behind_camera", C.c_int),
                ("trust_region_strategy", C.c_int)]


class CeresSummary(C.Structure):
    _fields_ = [("iterations", C.c_int), ("successful_steps", C.c_int), ("unsuccessful_steps", C.c_int),
                ("termination", C.c_int), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_radius", C.c_double)]


class BaStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("lm_trials", C.c_int), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
                ("lambda_final", C.c_double)]


class InitParams(C.Structure):
    _fields_ = [("sigma", C.c_float), ("sigma2", C.c_float), ("max_iter", C.c_int), ("min_parallax", C.c_double), ("min_triangulated", C.c_int),
                ("good_point_ratio_h", C.c_double)]


class InitResult(C.Structure):
    _fields_ = [("H21", C.c_double * 9), ("F21", C.c_double * 9), ("R21", C.c_double * 9), ("t21", C.c_double * 3), ("T21", C.c_double * 7),
                ("parallax", C.c_double), ("score_h", C.c_float), ("score_f", C.c_float), ("rh", C.c_float), ("success", C.c_int32),
                ("model", C.c_int32), ("best_h", C.c_int32), ("best_f", C.c_int32), ("n_inliers", C.c_int32), ("solution", C.c_int32),
                ("n_good", C.c_int32), ("second_good", C.c_int32), ("similar", C.c_int32), ("n_triangulated", C.c_int32)]

    def to_dict(self):
        d = {}
        for name, ty in self._fields_:
            v = getattr(self, name)
            d[name] = np.array(v[:]) if hasattr(ty, "_length_") else v
        return d


def default_init_params():
    p = InitParams()
    load().ygz_hip_default_init_params(C.byref(p))
    return p


def _init_params(**kw):
    p = default_init_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def init_sample_sets(n, max_iter=200):
    """the 8-point sample sets of Initializer::TryInitialize (Initializer.cpp:24-48): [max_iter][8], host only"""
    s = np.zeros((max(max_iter, 1), 8), np.int32)
    lib = load()
    lib.ygz_hip_init_sample_sets.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32)]
    rc = lib.ygz_hip_init_sample_sets(n, max_iter, _p(s, C.c_int32))
    if rc != OK:
        raise YgzHipError(rc, "init_sample_sets")
    return s


class PnpParams(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("chi2", C.c_double), ("min_inliers", C.c_int)]


class PnpResult(C.Structure):
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("T_cw", C.c_double * 7), ("success", C.c_int32), ("n_inliers", C.c_int32),
                ("best_sample", C.c_int32), ("best_solution", C.c_int32), ("n_hypotheses", C.c_int32)]

    def to_dict(self):
        return InitResult.to_dict(self)


def default_pnp_params():
    p = PnpParams()
    load().ygz_hip_default_pnp_params(C.byref(p))
    return p


def _pnp_params(**kw):
    p = default_pnp_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def pnp_sample_sets(n, max_iter=300):
    """the 3-point sample sets of the relocalisation's P3P RANSAC (Initializer.cpp:33-49's scheme): [max_iter][3], host only"""
    s = np.zeros((max(max_iter, 1), 3), np.int32)
    lib = load()
    lib.ygz_hip_pnp_sample_sets.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32)]
    rc = lib.ygz_hip_pnp_sample_sets(n, max_iter, _p(s, C.c_int32))
    if rc != OK:
        raise YgzHipError(rc, "pnp_sample_sets")
    return s


class Sim3Params(C.Structure):
    _fields_ = [("max_iter", C.c_int), ("chi2", C.c_double), ("min_inliers", C.c_int), ("chi2_refine", C.c_double), ("iters_first", C.c_int),
                ("iters_more", C.c_int), ("iters_again", C.c_int), ("fix_scale", C.c_int)]


class Sim3Result(C.Structure):
    _fields_ = [("S12", C.c_double * 8), ("S21", C.c_double * 8), ("chi2_ransac", C.c_double), ("chi2_refined", C.c_double),
                ("success", C.c_int32), ("n_hypotheses", C.c_int32), ("best_sample", C.c_int32), ("n_inliers", C.c_int32),
                ("n_refined", C.c_int32), ("lm_iterations", C.c_int32)]

    def to_dict(self):
        return InitResult.to_dict(self)


def default_sim3_params():
    p = Sim3Params()
    load().ygz_hip_default_sim3_params(C.byref(p))
    return p


def _sim3_params(**kw):
    p = default_sim3_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


class ProjProblem(C.Structure):
    """ygz_proj_problem (include/ygz_hip.h)"""
    _fields_ = [("kp_px", C.POINTER(C.c_double)), ("kp_level", C.POINTER(C.c_int32)), ("kp_desc", C.POINTER(C.c_uint8)),
                ("kp_taken", C.POINTER(C.c_uint8)), ("n_kp", C.c_int), ("pw", C.POINTER(C.c_double)), ("pt_desc", C.POINTER(C.c_uint8)),
                ("pt_dmax", C.POINTER(C.c_double)), ("pt_normal", C.POINTER(C.c_double)), ("pt_skip", C.POINTER(C.c_uint8)), ("n_pt", C.c_int),
                ("S", C.c_double * 8)]


class ProjParams(C.Structure):
    _fields_ = [("th", C.c_double), ("th_dist", C.c_int), ("claim", C.c_int)]


def default_proj_params():
    p = ProjParams()
    load().ygz_hip_default_proj_params(C.byref(p))
    return p


def _proj_params(**kw):
    p = default_proj_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def proj_problems(problems):
    """a ygz_proj_problem array from dicts (kp_px, kp_level, kp_desc, pw, pt_desc, pt_dmax, S; kp_taken, pt_normal, pt_skip optional or None;
    n_kp / n_pt override the array lengths) and the arrays that must outlive it"""
    arr = (ProjProblem * max(len(problems), 1))()
    keep = []
    for q, d in enumerate(problems):
        def get(name, dtype, shape, ctype):
            a = d.get(name)
            if a is None:                                   # a null pointer: optional, or for the library to refuse
                return C.POINTER(ctype)(), None
            a = np.ascontiguousarray(a, dtype).reshape(shape)
            keep.append(a)
            return _p(a, ctype), len(a)
        b = arr[q]
        b.kp_px, nk = get("kp_px", np.float64, (-1, 2), C.c_double)
        b.kp_level, n1 = get("kp_level", np.int32, (-1,), C.c_int32)
        b.kp_desc, n2 = get("kp_desc", np.uint8, (-1, 32), C.c_uint8)
        b.kp_taken, n3 = get("kp_taken", np.uint8, (-1,), C.c_uint8)
        b.pw, npt = get("pw", np.float64, (-1, 3), C.c_double)
        b.pt_desc, m1 = get("pt_desc", np.uint8, (-1, 32), C.c_uint8)
        b.pt_dmax, m2 = get("pt_dmax", np.float64, (-1,), C.c_double)
        b.pt_normal, m3 = get("pt_normal", np.float64, (-1, 3), C.c_double)
        b.pt_skip, m4 = get("pt_skip", np.uint8, (-1,), C.c_uint8)
        ks, ps = [v for v in (nk, n1, n2, n3) if v is not None], [v for v in (npt, m1, m2, m3, m4) if v is not None]
        if len(set(ks)) > 1 or len(set(ps)) > 1:
            raise ValueError("problem %d: arrays differ in length" % q)
        b.n_kp, b.n_pt = int(d.get("n_kp", ks[0] if ks else 0)), int(d.get("n_pt", ps[0] if ps else 0))
        if (ks and b.n_kp > ks[0]) or (ps and b.n_pt > ps[0]):
            raise ValueError("problem %d: n_kp / n_pt above the array lengths" % q)
        b.S = (C.c_double * 8)(*[float(v) for v in d["S"]])
    return arr, keep


class PgoParams(C.Structure):
    """ygz_pgo_params (include/ygz_hip.h)"""
    _fields_ = [("max_iterations", C.c_int32), ("max_trials", C.c_int32), ("cg_max_iterations", C.c_int32), ("fix_scale", C.c_int32),
                ("cg_tol", C.c_double), ("min_rel_decrease", C.c_double)]


class PgoResult(C.Structure):
    """ygz_pgo_result; `lambda_` is the header's `lambda`"""
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("lambda_", C.c_double), ("status", C.c_int32),
                ("lm_iterations", C.c_int32), ("n_solves", C.c_int32), ("cg_iterations_total", C.c_int32), ("cg_capped", C.c_int32),
                ("pad", C.c_int32)]

    def to_dict(self):
        return dict((k, getattr(self, k)) for k, _ in self._fields_ if k != "pad")


def default_pgo_params():
    p = PgoParams()
    load().ygz_hip_default_pgo_params(C.byref(p))
    return p


def _pgo_params(**kw):
    p = default_pgo_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def pgo_arrays(S, fixed, edges, M):
    """the four arrays of a pose graph in the ABI's types: S [N][8], fixed [N] uint8, edges [E][2] int32, M [E][8]"""
    S = np.ascontiguousarray(S, np.float64).reshape(-1, 8)
    M = np.ascontiguousarray(M, np.float64).reshape(-1, 8)
    fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
    if len(S) != len(fixed) or len(edges) != len(M):
        raise ValueError("S / fixed or edges / M differ in length")
    return S, fixed, edges, M


def pgo_argtypes(lib):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.ygz_hip_pose_graph_optimize.argtypes = [C.c_void_p, C.c_int, dp, C.POINTER(C.c_uint8), C.c_int, ip, dp, C.POINTER(PgoParams), dp,
                                                C.POINTER(PgoResult)]
    lib.ygz_hip_pgo_linearize.argtypes = [C.c_void_p, C.c_int, dp, C.POINTER(C.c_uint8), C.c_int, ip, dp, C.POINTER(PgoParams), dp, dp, dp, dp]


class GbaParams(C.Structure):
    """ygz_gba_params (include/ygz_hip.h)"""
    _fields_ = [("max_iterations", C.c_int32), ("max_trials", C.c_int32), ("cg_max_iterations", C.c_int32), ("cg_batch", C.c_int32),
                ("cg_tol", C.c_double), ("min_rel_decrease", C.c_double)]


class GbaResult(C.Structure):
    """ygz_gba_result; `lambda_` is the header's `lambda`"""
    _fields_ = [("cost_initial", C.c_double), ("cost_final", C.c_double), ("lambda_", C.c_double), ("status", C.c_int32),
                ("lm_iterations", C.c_int32), ("n_solves", C.c_int32), ("cg_iterations_total", C.c_int32), ("cg_capped", C.c_int32),
                ("pad", C.c_int32)]

    def to_dict(self):
        return dict((k, getattr(self, k)) for k, _ in self._fields_ if k != "pad")


def default_gba_params():
    p = GbaParams()
    load().ygz_hip_default_gba_params(C.byref(p))
    return p


def _gba_params(**kw):
    p = default_gba_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def gba_arrays(poses, fixed, points, edge_pose, edge_point, obs):
    """the six arrays of a bundle-adjustment problem in the ABI's types: poses [N][7], fixed [N] uint8, points [L][3], edge_pose and
    edge_point [E] int32, obs [E][2]"""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
    points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 2)
    fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    edge_pose = np.ascontiguousarray(edge_pose, np.int32).reshape(-1)
    edge_point = np.ascontiguousarray(edge_point, np.int32).reshape(-1)
    if len(poses) != len(fixed) or not len(edge_pose) == len(edge_point) == len(obs):
        raise ValueError("poses / fixed or edge_pose / edge_point / obs differ in length")
    return poses, fixed, points, edge_pose, edge_point, obs


def gba_argtypes(lib):
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    problem = [C.c_void_p, C.c_int, dp, bp, C.c_int, dp, C.c_int, ip, ip, dp, dp, C.c_double, C.POINTER(GbaParams)]
    lib.ygz_hip_global_ba.argtypes = problem + [dp, dp, C.POINTER(GbaResult)]
    lib.ygz_hip_gba_linearize.argtypes = problem + [dp] * 9


class SbaParams(C.Structure):
    """ygz_sba_params (include/ygz_hip.h)"""
    _fields_ = [("max_iterations", C.c_int32), ("max_trials", C.c_int32), ("cg_max_iterations", C.c_int32), ("cg_batch", C.c_int32),
                ("cg_tol", C.c_double), ("min_rel_decrease", C.c_double), ("baseline", C.c_double), ("chi2_mono", C.c_double),
                ("chi2_stereo", C.c_double), ("rounds", C.c_int32), ("robust_rounds", C.c_int32), ("iterations", C.c_int32 * 4)]


class SbaResult(C.Structure):
    """ygz_sba_result; `lambda_` is the header's `lambda`"""
    _fields_ = [("cost_initial", C.c_double * 4), ("cost_final", C.c_double * 4), ("lambda_", C.c_double * 4), ("rounds_run", C.c_int32),
                ("launches", C.c_int32), ("status", C.c_int32 * 4), ("lm_iterations", C.c_int32 * 4), ("n_solves", C.c_int32 * 4),
                ("cg_iterations", C.c_int32 * 4), ("cg_capped", C.c_int32 * 4), ("inliers", C.c_int32 * 4)]

    def to_dict(self):
        return dict((k, getattr(self, k) if k in ("rounds_run", "launches") else np.array(getattr(self, k))) for k, _ in self._fields_)


def default_sba_params():
    p = SbaParams()
    load().ygz_hip_default_sba_params(C.byref(p))
    return p


def _sba_params(**kw):
    p = default_sba_params()
    for k, v in kw.items():
        if v is None:
            continue
        if k == "iterations":
            v = list(v) + [0] * (4 - len(v))
            for i in range(4):
                p.iterations[i] = int(v[i])
        else:
            setattr(p, k, v)
    return p


def sba_arrays(poses, fixed, points, edge_pose, edge_point, obs, kind, level):
    """the eight arrays of a stereo bundle-adjustment problem in the ABI's types: gba_arrays' with obs [E][3], kind [E] uint8, level [E] int32"""
    obs = np.ascontiguousarray(obs, np.float64).reshape(-1, 3)
    poses, fixed, points, edge_pose, edge_point, _ = gba_arrays(poses, fixed, points, edge_pose, edge_point, obs[:, :2])
    kind = np.ascontiguousarray(kind, np.uint8).reshape(-1)
    level = np.ascontiguousarray(level, np.int32).reshape(-1)
    if not len(kind) == len(level) == len(obs):
        raise ValueError("kind / level / obs differ in length")
    return poses, fixed, points, edge_pose, edge_point, obs, kind, level


def sba_argtypes(lib):
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    problem = [C.c_void_p, C.c_int, dp, bp, C.c_int, dp, C.c_int, ip, ip, dp, bp, ip, dp, C.POINTER(SbaParams)]
    lib.ygz_hip_stereo_ba.argtypes = problem + [dp, dp, bp, dp, C.POINTER(SbaResult)]
    lib.ygz_hip_sba_linearize.argtypes = problem + [dp] * 9


def kfdb_argtypes(lib):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.ygz_hip_kfdb_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.ygz_hip_kfdb_destroy.argtypes = [C.c_void_p]
    lib.ygz_hip_kfdb_destroy.restype = None
    lib.ygz_hip_kfdb_add.argtypes = [C.c_void_p, ip, dp, C.c_int, ip]
    lib.ygz_hip_kfdb_erase.argtypes = [C.c_void_p, C.c_int32]
    lib.ygz_hip_kfdb_clear.argtypes = [C.c_void_p]
    lib.ygz_hip_kfdb_info.argtypes = [C.c_void_p, ip, ip, C.POINTER(C.c_int64)]
    lib.ygz_hip_kfdb_query.argtypes = [C.c_void_p, C.c_int, ip, ip, dp, ip, dp]


def kfdb_pack(vectors):
    """a list of (word, weight) pairs as the ABI's q_offsets [n + 1], q_word and q_weight (arrays of at least one element)"""
    off = np.zeros(len(vectors) + 1, np.int32)
    off[1:] = np.cumsum([len(w) for w, _ in vectors])
    word = np.ascontiguousarray(np.concatenate([np.asarray(w, np.int32).reshape(-1) for w, _ in vectors] + [np.zeros(1, np.int32)]))
    weight = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).reshape(-1) for _, v in vectors] + [np.zeros(1)]))
    return off, word, weight


def map_argtypes(lib):
    ip, bp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    lib.ygz_hip_distinctive_descriptors.argtypes = [C.c_void_p, C.c_int, ip, bp, ip, ip, bp]
    lib.ygz_hip_covisibility.argtypes = [C.c_void_p, C.c_int, ip, ip, C.c_int, C.c_int, ip, ip]


class CullParams(C.Structure):
    """ygz_cull_params (include/ygz_hip.h)"""
    _fields_ = [("th_obs", C.c_int32), ("level_slack", C.c_int32), ("min_obs", C.c_int32), ("pad", C.c_int32), ("ratio", C.c_double)]


def default_cull_params():
    p = CullParams()
    load().ygz_hip_default_cull_params(C.byref(p))
    return p


def _cull_params(**kw):
    p = default_cull_params()
    for k, v in kw.items():
        if v is not None:
            setattr(p, k, v)
    return p


def cull_argtypes(lib):
    ip, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(CullParams)
    lib.ygz_hip_default_cull_params.argtypes = [pp]
    lib.ygz_hip_default_cull_params.restype = None
    lib.ygz_hip_keyframe_redundancy.argtypes = [C.c_void_p, C.c_int, ip, ip, ip, C.c_int, pp, ip, ip]
    lib.ygz_hip_cull_keyframes.argtypes = [C.c_void_p, C.c_int, ip, ip, ip, C.c_int, C.c_int, ip, pp, ip, ip, ip, bp]


def cull_arrays(offsets, kf, level):
    """the three arrays of the observation lists in the ABI's types (kf and level of at least one element)"""
    off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
    k = np.ascontiguousarray(kf, np.int32).reshape(-1)
    l = np.ascontiguousarray(level, np.int32).reshape(-1)
    if len(off) < 2 or int(off[-1]) != len(k) or len(k) != len(l):
        raise ValueError("offsets do not describe kf and level")
    if not len(k):
        k, l = np.zeros(1, np.int32), np.zeros(1, np.int32)
    return off, k, l


class UndistortParams(C.Structure):
    """ygz_undistort_params (include/ygz_hip.h)"""
    _fields_ = [("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("k3", C.c_double),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("border_value", C.c_int)]


def undistort_argtypes(lib):
    ip, pp = C.POINTER(C.c_int32), C.POINTER(UndistortParams)
    lib.ygz_hip_default_undistort_params.argtypes = [C.c_void_p, pp]
    lib.ygz_hip_set_undistortion.argtypes = [C.c_void_p, pp]
    lib.ygz_hip_undistort_map.argtypes = [C.c_void_p, ip, ip]
    lib.ygz_hip_build_pyramid_undistorted.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]


class RectifyParams(C.Structure):
    """ygz_rectify_params (include/ygz_hip.h)"""
    _fields_ = [("lens", UndistortParams), ("R", C.c_double * 9)]


def rectify_argtypes(lib):
    ip, dp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(RectifyParams)
    lib.ygz_hip_stereo_rectify.argtypes = [dp, dp, dp, dp, dp]
    lib.ygz_hip_default_rectify_params.argtypes = [C.c_void_p, pp]
    lib.ygz_hip_set_rectification.argtypes = [C.c_void_p, C.c_int, pp]
    lib.ygz_hip_rectify_map.argtypes = [C.c_void_p, C.c_int, ip, ip]
    lib.ygz_hip_build_pyramid_rectified.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8)]


def stereo_rectify(R, T):
    """ygz_hip_stereo_rectify (host code, no device): (R1 [3, 3], R2 [3, 3], baseline) of the rig X_right = R X_left + T; RuntimeError when
    the rig is refused"""
    lib = load()
    rectify_argtypes(lib)
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    T = np.ascontiguousarray(T, np.float64).reshape(3)
    R1, R2, b = np.zeros(9), np.zeros(9), C.c_double(0)
    rc = lib.ygz_hip_stereo_rectify(_p(R, C.c_double), _p(T, C.c_double), _p(R1, C.c_double), _p(R2, C.c_double), C.byref(b))
    if rc != 0:
        raise RuntimeError("ygz_hip_stereo_rectify: error %d" % rc)
    return R1.reshape(3, 3), R2.reshape(3, 3), b.value


class StereoParams(C.Structure):
    """ygz_stereo_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("min_disparity", C.c_double), ("max_disparity", C.c_double), ("th_dist", C.c_int), ("write_depths", C.c_int)]


def stereo_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(StereoParams)
    lib.ygz_hip_default_stereo_params.argtypes = [pp]
    lib.ygz_hip_default_stereo_params.restype = None
    lib.ygz_hip_stereo_depths_slots.argtypes = [C.c_void_p, C.c_int, ip, ip, pp, ip, dp, dp, ip, ip, ip]
    arrays = [C.c_void_p, C.c_int, C.c_int, dp, ip, bp, C.c_int, dp, ip, bp, C.c_int, pp]
    lib.ygz_hip_stereo_match.argtypes = arrays + [ip, dp, dp, ip, ip, ip]
    lib.ygz_hip_stereo_candidates.argtypes = arrays + [ip, ip, ip, ip]


class PoseOptParams(C.Structure):
    """ygz_pose_opt_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("chi2_mono", C.c_double), ("chi2_stereo", C.c_double), ("rounds", C.c_int), ("iterations", C.c_int),
                ("max_trials", C.c_int), ("robust_rounds", C.c_int), ("min_edges", C.c_int), ("min_inliers", C.c_int), ("min_rel_decrease", C.c_double)]


def popt_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(PoseOptParams)
    lib.ygz_hip_default_pose_opt_params.argtypes = [pp]
    lib.ygz_hip_default_pose_opt_params.restype = None
    lib.ygz_hip_optimize_pose_stereo.argtypes = [C.c_void_p, C.c_int, ip, dp, dp, ip, bp, pp, dp, bp, dp, ip, ip, ip, ip, dp, dp, dp]


class SmapParams(C.Structure):
    """ygz_smap_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("chi2_mono", C.c_double), ("chi2_stereo", C.c_double), ("cos_parallax_max", C.c_double),
                ("ratio_factor", C.c_double), ("th_depth", C.c_double), ("min_close", C.c_int32), ("pad", C.c_int32)]


class SmapProblem(C.Structure):
    """ygz_smap_problem (include/ygz_hip.h)"""
    _fields_ = [("T1", C.c_double * 7), ("T2", C.c_double * 7), ("px1", C.POINTER(C.c_double)), ("px2", C.POINTER(C.c_double)),
                ("ur1", C.POINTER(C.c_double)), ("ur2", C.POINTER(C.c_double)), ("depth1", C.POINTER(C.c_double)), ("depth2", C.POINTER(C.c_double)),
                ("level1", C.POINTER(C.c_int32)), ("level2", C.POINTER(C.c_int32)), ("n", C.c_int)]


def smap_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(SmapParams)
    cp = C.POINTER(C.c_int)
    lib.ygz_hip_default_smap_params.argtypes = [pp]
    lib.ygz_hip_default_smap_params.restype = None
    lib.ygz_hip_stereo_create_map_points.argtypes = [C.c_void_p, C.c_int, C.POINTER(SmapProblem), dp, pp, ip, ip, dp, ip]
    lib.ygz_hip_stereo_keyframe_points.argtypes = [C.c_void_p, dp, C.c_int, dp, dp, bp, dp, pp, ip, bp, dp, cp, cp, cp]


class LfuseParams(C.Structure):
    """ygz_lfuse_params (include/ygz_hip.h)"""
    _fields_ = [("th", C.c_double), ("baseline", C.c_double), ("chi2_mono", C.c_double), ("chi2_stereo", C.c_double), ("th_dist", C.c_int32),
                ("pad", C.c_int32)]


class LfusePoints(C.Structure):
    """ygz_lfuse_points (include/ygz_hip.h)"""
    _fields_ = [("pw", C.POINTER(C.c_double)), ("pt_desc", C.POINTER(C.c_uint8)), ("pt_dmax", C.POINTER(C.c_double)),
                ("pt_normal", C.POINTER(C.c_double)), ("n_pt", C.c_int)]


class LfuseProblem(C.Structure):
    """ygz_lfuse_problem (include/ygz_hip.h)"""
    _fields_ = [("T", C.c_double * 7), ("kp_px", C.POINTER(C.c_double)), ("kp_level", C.POINTER(C.c_int32)), ("kp_desc", C.POINTER(C.c_uint8)),
                ("kp_ur", C.POINTER(C.c_double)), ("kp_taken", C.POINTER(C.c_uint8)), ("pt_skip", C.POINTER(C.c_uint8)), ("n_kp", C.c_int),
                ("set", C.c_int)]


def lfuse_argtypes(lib):
    ip, dp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(LfuseParams)
    lib.ygz_hip_default_lfuse_params.argtypes = [pp]
    lib.ygz_hip_default_lfuse_params.restype = None
    lib.ygz_hip_local_fuse_search.argtypes = [C.c_void_p, C.c_int, C.POINTER(LfusePoints), C.c_int, C.POINTER(LfuseProblem), dp, pp,
                                              ip, ip, ip, ip, ip, ip]


class StrackParams(C.Structure):
    """ygz_strack_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("ratio", C.c_double), ("r_near", C.c_double), ("r_wide", C.c_double), ("cos_near", C.c_double),
                ("th_dist", C.c_int32), ("check_orientation", C.c_int32)]


class StrackPoints(C.Structure):
    """ygz_strack_points (include/ygz_hip.h)"""
    _fields_ = [("pw", C.POINTER(C.c_double)), ("pt_desc", C.POINTER(C.c_uint8)), ("pt_level", C.POINTER(C.c_int32)),
                ("pt_angle", C.POINTER(C.c_double)), ("pt_dmax", C.POINTER(C.c_double)), ("pt_normal", C.POINTER(C.c_double)), ("n_pt", C.c_int)]


class StrackProblem(C.Structure):
    """ygz_strack_problem (include/ygz_hip.h)"""
    _fields_ = [("T", C.c_double * 7), ("th", C.c_double), ("kp_px", C.POINTER(C.c_double)), ("kp_level", C.POINTER(C.c_int32)),
                ("kp_desc", C.POINTER(C.c_uint8)), ("kp_ur", C.POINTER(C.c_double)), ("kp_angle", C.POINTER(C.c_double)),
                ("kp_taken", C.POINTER(C.c_uint8)), ("pt_skip", C.POINTER(C.c_uint8)), ("n_kp", C.c_int), ("set", C.c_int), ("mode", C.c_int),
                ("direction", C.c_int)]


def strack_argtypes(lib):
    ip, dp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(StrackParams)
    lib.ygz_hip_default_strack_params.argtypes = [pp]
    lib.ygz_hip_default_strack_params.restype = None
    lib.ygz_hip_stereo_track_search.argtypes = [C.c_void_p, C.c_int, C.POINTER(StrackPoints), C.c_int, C.POINTER(StrackProblem), dp, pp,
                                                ip, ip, ip, ip, ip, ip, ip, dp, ip, ip, ip]


class SvoParams(C.Structure):
    """ygz_svo_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("th", C.c_double), ("th_dist", C.c_int32), ("check_orientation", C.c_int32),
                ("min_matches", C.c_int32), ("pad", C.c_int32), ("pose", PoseOptParams)]


def svo_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(SvoParams)
    lib.ygz_hip_default_svo_params.argtypes = [pp]
    lib.ygz_hip_default_svo_params.restype = None
    lib.ygz_hip_stereo_odometry_slots.argtypes = [C.c_void_p, C.c_int, ip, ip, dp, ip, pp, dp, ip, ip, ip, ip, ip, ip, ip, ip, ip, dp, ip, bp, dp,
                                                  ip, ip, ip, ip, dp, dp, dp]


class SlmParams(C.Structure):
    """ygz_slm_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("th", C.c_double), ("ratio", C.c_double), ("r_near", C.c_double), ("r_wide", C.c_double),
                ("cos_near", C.c_double), ("th_dist", C.c_int32), ("min_edges", C.c_int32), ("pose", PoseOptParams)]


def slm_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(SlmParams)
    lib.ygz_hip_default_slm_params.argtypes = [pp]
    lib.ygz_hip_default_slm_params.restype = None
    lib.ygz_hip_stereo_local_map_slots.argtypes = [C.c_void_p, C.c_int, C.POINTER(StrackPoints), C.c_int, ip, ip, dp, ip, pp, dp, ip, ip, ip, bp, dp,
                                                   ip, ip, ip, ip, dp, dp, dp, ip, ip, ip, ip, ip, ip, ip, dp]


class SrkParams(C.Structure):
    """ygz_srk_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("th_low", C.c_int32), ("knn_ratio", C.c_float), ("levelsup", C.c_int32),
                ("check_orientation", C.c_int32), ("min_matches", C.c_int32), ("min_inliers", C.c_int32), ("pose", PoseOptParams)]


def srk_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(SrkParams)
    lib.ygz_hip_default_srk_params.argtypes = [pp]
    lib.ygz_hip_default_srk_params.restype = None
    lib.ygz_hip_stereo_ref_keyframe_slots.argtypes = [C.c_void_p, C.c_int, C.POINTER(StrackPoints), C.c_int, ip, ip, ip, C.c_int, ip, ip, dp, pp,
                                                      dp, ip, ip, ip, ip, bp, dp, ip, ip, ip, ip, dp, dp, dp, ip, ip, ip]


class SrlParams(C.Structure):
    """ygz_srl_params (include/ygz_hip.h)"""
    _fields_ = [("baseline", C.c_double), ("th_low", C.c_int32), ("knn_ratio", C.c_float), ("levelsup", C.c_int32),
                ("check_orientation", C.c_int32), ("min_matches", C.c_int32), ("pad0", C.c_int32), ("pnp", PnpParams),
                ("min_final_inliers", C.c_int32), ("pad1", C.c_int32), ("pose", PoseOptParams)]


def srl_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(SrlParams)
    lib.ygz_hip_default_srl_params.argtypes = [pp]
    lib.ygz_hip_default_srl_params.restype = None
    lib.ygz_hip_stereo_relocalize_slots.argtypes = [C.c_void_p, C.c_int, C.POINTER(StrackPoints), C.c_int, ip, ip, ip, C.c_int, ip, ip, ip, pp,
                                                    dp, ip, ip, dp, dp, C.POINTER(PnpResult), ip, ip, ip, ip, ip, dp, dp, dp, ip, ip, bp, ip, bp,
                                                    dp, ip, ip, ip]


class LmsParams(C.Structure):
    """ygz_lms_params (include/ygz_hip.h)"""
    _fields_ = [("max_keyframes", C.c_int32), ("max_points", C.c_int32)]


def lms_argtypes(lib):
    ip, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(LmsParams)
    lib.ygz_hip_default_lms_params.argtypes = [pp]
    lib.ygz_hip_default_lms_params.restype = None
    lib.ygz_hip_local_map_select.argtypes = [C.c_void_p, C.c_int, bp, C.c_int, ip, C.c_int, ip, ip, ip, bp, C.c_int, ip, ip, pp] + [ip] * 9


def mpa_argtypes(lib):
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.ygz_hip_map_point_attributes.argtypes = [C.c_void_p, C.c_int, dp, C.c_int, dp, ip, ip, ip, dp, dp, ip]


def slm_indexed_argtypes(lib):
    ip, dp, bp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(SlmParams)
    lib.ygz_hip_stereo_local_map_indexed.argtypes = [C.c_void_p, C.c_int, dp, bp, dp, dp, C.c_int, C.c_int, ip, ip, C.c_int, ip, ip, dp, ip, pp, dp,
                                                     ip, ip, ip, bp, dp, ip, ip, ip, ip, dp, dp, dp, ip, ip, ip, ip, ip, ip, ip, dp]


class MapArrays(C.Structure):
    _fields_ = [("n_keyframes", C.c_int32), ("n_cov", C.c_int32), ("n_points", C.c_int32), ("n_centres", C.c_int32),
                ("kf_bad", C.POINTER(C.c_uint8)), ("cov", C.POINTER(C.c_int32)), ("offsets", C.POINTER(C.c_int32)), ("kf", C.POINTER(C.c_int32)),
                ("feat", C.POINTER(C.c_int32)), ("pt_bad", C.POINTER(C.c_uint8)), ("centre", C.POINTER(C.c_double)),
                ("a_offsets", C.POINTER(C.c_int32)), ("a_kf", C.POINTER(C.c_int32)), ("a_level", C.POINTER(C.c_int32)),
                ("pw", C.POINTER(C.c_double)), ("pt_desc", C.POINTER(C.c_uint8)), ("pt_has_desc", C.POINTER(C.c_uint8))]


class MapInfo(C.Structure):
    _fields_ = [("n_keyframes", C.c_int32), ("n_cov", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("n_centres", C.c_int32),
                ("n_rows", C.c_int32), ("uploads", C.c_int32), ("updates", C.c_int32), ("resident_bytes", C.c_uint64)]


def rmap_argtypes(lib):
    ip, dp, bp, vp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_void_p
    lib.ygz_hip_map_create.argtypes = [vp, C.POINTER(vp)]
    lib.ygz_hip_map_destroy.argtypes = [vp, vp]
    lib.ygz_hip_map_info.argtypes = [vp, vp, C.POINTER(MapInfo)]
    lib.ygz_hip_map_upload.argtypes = [vp, vp, C.POINTER(MapArrays), dp, dp, ip]
    lib.ygz_hip_map_update.argtypes = [vp, vp, C.c_int, ip, dp, bp, bp, bp, C.c_int, ip, bp, C.c_int, ip, dp]
    lib.ygz_hip_map_download.argtypes = [vp, vp, dp, bp, bp, bp, bp, dp, dp, dp, ip]
    lib.ygz_hip_stereo_local_map_resident.argtypes = [vp, vp, C.c_int, ip, dp, ip, ip, C.POINTER(LmsParams), C.POINTER(SlmParams)] + [ip] * 10 + [
        dp, ip, ip, ip, bp, dp, ip, ip, ip, ip, dp, dp, dp, ip, ip, ip, ip, ip, ip, ip, dp]


# every symbol include/ygz_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "ygz_hip_default_params", "ygz_hip_create", "ygz_hip_destroy", "ygz_hip_synchronize", "ygz_hip_join", "ygz_hip_set_overlap", "ygz_hip_error_string",
    "ygz_hip_last_hip_error", "ygz_hip_max_keypoints", "ygz_hip_timer_begin", "ygz_hip_timer_end", "ygz_hip_probe_begin", "ygz_hip_probe_end",
    "ygz_hip_upload_bgr", "ygz_hip_upload_gray", "ygz_hip_build_pyramid", "ygz_hip_download_level", "ygz_hip_download_framed_level", "ygz_hip_level_size",
    "ygz_hip_detect", "ygz_hip_keypoint_count", "ygz_hip_get_keypoints", "ygz_hip_describe", "ygz_hip_describe_given_angle", "ygz_hip_get_fast_maps",
    "ygz_hip_match_slots", "ygz_hip_match_slots_again", "ygz_hip_get_matches", "ygz_hip_hamming_match",
    "ygz_hip_find_direct_projection", "ygz_hip_align2d", "ygz_hip_sparse_align", "ygz_hip_sparse_align_residuals",
    "ygz_hip_default_klt_params", "ygz_hip_klt_track", "ygz_hip_klt_track_filtered",
    "ygz_hip_set_keypoint_depths", "ygz_hip_track_begin", "ygz_hip_track_reload", "ygz_hip_track_klt", "ygz_hip_track_klt_prepare", "ygz_hip_track_direct",
    "ygz_hip_track_sparse_align", "ygz_hip_track_get_klt", "ygz_hip_track_get_direct", "ygz_hip_track_get_pose",
    "ygz_hip_ba_linearize", "ygz_hip_ba_upload", "ygz_hip_ba_set_state", "ygz_hip_ba_set_state_device", "ygz_hip_ba_linearize_resident", "ygz_hip_ba_download", "ygz_hip_ba_optimize",
    "ygz_hip_ba_optimize_resident", "ygz_hip_ba_set_team_budget", "ygz_hip_ba_get_state", "ygz_hip_ba_behind_camera", "ygz_hip_ba_set_enable", "ygz_hip_ba_light_barrier", "ygz_hip_ceres_default_options", "ygz_hip_ba_solve_ceres", "ygz_hip_ba_solve_ceres_resident", "ygz_hip_optimize_pose_only",
    "ygz_hip_vocab_load", "ygz_hip_vocab_info", "ygz_hip_compute_bow", "ygz_hip_get_bow", "ygz_hip_bow_transform", "ygz_hip_search_by_bow_slots", "ygz_hip_search_by_bow", "ygz_hip_depth_from_triangulation", "ygz_hip_track_local_map", "ygz_hip_find_direct_projection_mp", "ygz_hip_find_direct_projection_mp_begin", "ygz_hip_find_direct_projection_mp_end", "ygz_hip_set_wait_hook",
    "ygz_hip_match_postfilter", "ygz_hip_get_good_matches", "ygz_hip_match_postfilter_host", "ygz_hip_match_sets", "ygz_hip_check_frame_descriptors",
    "ygz_hip_check_descriptor_pairs", "ygz_hip_track_adopt_pose", "ygz_hip_track_pose_only", "ygz_hip_track_get_pose_only",
    "ygz_hip_pinned_alloc", "ygz_hip_pinned_free", "ygz_hip_upload_bgr_batch", "ygz_hip_upload_gray_batch", "ygz_hip_get_keypoint_pixels_batch",
    "ygz_hip_get_keypoints_batch", "ygz_hip_set_keypoint_depths_batch", "ygz_hip_track_get_summary", "ygz_hip_create_map_points", "ygz_hip_depth_filter_update",
    "ygz_hip_get_keypoint_counts", "ygz_hip_get_keypoint_depths", "ygz_hip_upload_depth_batch", "ygz_hip_keypoint_depths_from_image", "ygz_hip_ba_get_stats", "ygz_hip_se3_chain", "ygz_hip_stream_wait", "ygz_hip_mark", "ygz_hip_wait_mark",
    "ygz_hip_kf_row_bytes", "ygz_hip_kf_store_create", "ygz_hip_kf_store_info", "ygz_hip_kf_store_put", "ygz_hip_kf_store_put_trel",
    "ygz_hip_kf_store_set_trel", "ygz_hip_kf_store_refresh", "ygz_hip_ba_reserve_windows", "ygz_hip_ba_build_windows", "ygz_hip_ba_pack_states", "ygz_hip_ba_mark_outliers", "ygz_hip_ba_get_outlier_stats", "ygz_hip_bow_orientation", "ygz_hip_bow_orientation_slots", "ygz_hip_ba_last_path",
    "ygz_hip_abi_version", "ygz_hip_ba_optimize_chi2", "ygz_hip_ba_set_team_placement", "ygz_hip_get_stream", "ygz_hip_get_device", "ygz_hip_make_current", "ygz_hip_device_alloc", "ygz_hip_device_free", "ygz_hip_copy",
    "ygz_hip_default_init_params", "ygz_hip_initialize", "ygz_hip_init_sample_sets", "ygz_hip_init_hypotheses", "ygz_hip_init_reconstruct",
    "ygz_hip_default_pnp_params", "ygz_hip_pnp_sample_sets", "ygz_hip_pnp_ransac", "ygz_hip_pnp_hypotheses",
    "ygz_hip_default_sim3_params", "ygz_hip_sim3_ransac", "ygz_hip_sim3_hypotheses",
    "ygz_hip_default_proj_params", "ygz_hip_search_by_projection", "ygz_hip_projection_candidates",
    "ygz_hip_default_pgo_params", "ygz_hip_pose_graph_optimize", "ygz_hip_pgo_linearize",
    "ygz_hip_distinctive_descriptors", "ygz_hip_covisibility",
    "ygz_hip_default_gba_params", "ygz_hip_global_ba", "ygz_hip_gba_linearize",
    "ygz_hip_default_sba_params", "ygz_hip_stereo_ba", "ygz_hip_sba_linearize",
    "ygz_hip_kfdb_create", "ygz_hip_kfdb_destroy", "ygz_hip_kfdb_add", "ygz_hip_kfdb_erase", "ygz_hip_kfdb_clear", "ygz_hip_kfdb_info", "ygz_hip_kfdb_query",
    "ygz_hip_default_cull_params", "ygz_hip_keyframe_redundancy", "ygz_hip_cull_keyframes",
    "ygz_hip_default_undistort_params", "ygz_hip_set_undistortion", "ygz_hip_undistort_map", "ygz_hip_build_pyramid_undistorted",
    "ygz_hip_default_stereo_params", "ygz_hip_stereo_depths_slots", "ygz_hip_stereo_match", "ygz_hip_stereo_candidates",
    "ygz_hip_default_pose_opt_params", "ygz_hip_optimize_pose_stereo",
    "ygz_hip_stereo_rectify", "ygz_hip_default_rectify_params", "ygz_hip_set_rectification", "ygz_hip_rectify_map", "ygz_hip_build_pyramid_rectified",
    "ygz_hip_default_smap_params", "ygz_hip_stereo_create_map_points", "ygz_hip_stereo_keyframe_points",
    "ygz_hip_default_lfuse_params", "ygz_hip_local_fuse_search",
    "ygz_hip_default_strack_params", "ygz_hip_stereo_track_search",
    "ygz_hip_default_svo_params", "ygz_hip_stereo_odometry_slots",
    "ygz_hip_default_slm_params", "ygz_hip_stereo_local_map_slots",
    "ygz_hip_default_srk_params", "ygz_hip_stereo_ref_keyframe_slots",
    "ygz_hip_default_srl_params", "ygz_hip_stereo_relocalize_slots",
    "ygz_hip_default_lms_params", "ygz_hip_local_map_select",
    "ygz_hip_map_point_attributes", "ygz_hip_stereo_local_map_indexed",
    "ygz_hip_map_create", "ygz_hip_map_destroy", "ygz_hip_map_info", "ygz_hip_map_upload", "ygz_hip_map_update", "ygz_hip_map_download",
    "ygz_hip_stereo_local_map_resident",
]
INIT_SYMBOLS = ["ygz_hip_default_init_params", "ygz_hip_initialize", "ygz_hip_init_sample_sets", "ygz_hip_init_hypotheses", "ygz_hip_init_reconstruct"]
INIT_NONE, INIT_H, INIT_F = 0, 1, 2
PNP_SYMBOLS = ["ygz_hip_default_pnp_params", "ygz_hip_pnp_sample_sets", "ygz_hip_pnp_ransac", "ygz_hip_pnp_hypotheses"]
PNP_MAX_ITER, PNP_MAX_PROBLEMS = 1024, 64
SIM3_SYMBOLS = ["ygz_hip_default_sim3_params", "ygz_hip_sim3_ransac", "ygz_hip_sim3_hypotheses"]
SIM3_MAX_ITER, SIM3_MAX_PROBLEMS = 1024, 64
PROJ_SYMBOLS = ["ygz_hip_default_proj_params", "ygz_hip_search_by_projection", "ygz_hip_projection_candidates"]
PROJ_MAX_PROBLEMS, PROJ_TOPK, PROJ_MAX_POINTS = 64, 8, 65536
PGO_SYMBOLS = ["ygz_hip_default_pgo_params", "ygz_hip_pose_graph_optimize", "ygz_hip_pgo_linearize"]
PGO_MAX_VERTICES, PGO_MAX_EDGES = 4096, 32768
PGO_FAILED, PGO_CONVERGED, PGO_MAX_ITERATIONS, PGO_STALLED = 0, 1, 2, 3
MAP_SYMBOLS = ["ygz_hip_distinctive_descriptors", "ygz_hip_covisibility"]
MAP_MAX_OBS_PER_POINT, MAP_MAX_OBS, MAP_MAX_KEYFRAMES, COVIS_MAX_CELLS = 256, 1048576, 4096, 4194304

GBA_SYMBOLS = ["ygz_hip_default_gba_params", "ygz_hip_global_ba", "ygz_hip_gba_linearize"]
GBA_MAX_POSES, GBA_MAX_POINTS, GBA_MAX_EDGES = 4096, 1048576, 4194304
GBA_FAILED, GBA_CONVERGED, GBA_MAX_ITERATIONS, GBA_STALLED = 0, 1, 2, 3
GBA_HUBER = 5.991

SBA_SYMBOLS = ["ygz_hip_default_sba_params", "ygz_hip_stereo_ba", "ygz_hip_sba_linearize"]
SBA_MAX_ROUNDS = 4

KFDB_SYMBOLS = ["ygz_hip_kfdb_create", "ygz_hip_kfdb_destroy", "ygz_hip_kfdb_add", "ygz_hip_kfdb_erase", "ygz_hip_kfdb_clear", "ygz_hip_kfdb_info",
                "ygz_hip_kfdb_query"]
KFDB_MAX_ENTRIES, KFDB_MAX_WORDS, KFDB_MAX_QUERIES = 4096, 8192, 64

CULL_SYMBOLS = ["ygz_hip_default_cull_params", "ygz_hip_keyframe_redundancy", "ygz_hip_cull_keyframes"]
CULL_MAX_KEYFRAMES = 4096

UNDISTORT_SYMBOLS = ["ygz_hip_default_undistort_params", "ygz_hip_set_undistortion", "ygz_hip_undistort_map", "ygz_hip_build_pyramid_undistorted"]
UNDISTORT_OUTSIDE = -2 ** 31

RECTIFY_SYMBOLS = ["ygz_hip_stereo_rectify", "ygz_hip_default_rectify_params", "ygz_hip_set_rectification", "ygz_hip_rectify_map",
                   "ygz_hip_build_pyramid_rectified"]
RECT_CAMERAS = 2

STEREO_SYMBOLS = ["ygz_hip_default_stereo_params", "ygz_hip_stereo_depths_slots", "ygz_hip_stereo_match", "ygz_hip_stereo_candidates"]
STEREO_OK, STEREO_NO_CANDIDATE, STEREO_DESCRIPTOR, STEREO_BORDER, STEREO_EDGE, STEREO_DISPARITY, STEREO_MEDIAN = range(7)
STEREO_N_STATUS, STEREO_COLUMNS = 7, 11

SMAP_SYMBOLS = ["ygz_hip_default_smap_params", "ygz_hip_stereo_create_map_points", "ygz_hip_stereo_keyframe_points"]
SMAP_MAX_PROBLEMS, SMAP_MAX_PAIRS = 32, 65536

LFUSE_SYMBOLS = ["ygz_hip_default_lfuse_params", "ygz_hip_local_fuse_search"]
LFUSE_MAX_PROBLEMS, LFUSE_MAX_SETS, LFUSE_MAX_PAIRS = 64, 8, 1048576
LFUSE_SEARCHED, LFUSE_SKIP, LFUSE_BEHIND, LFUSE_OUTSIDE, LFUSE_RANGE, LFUSE_ANGLE = range(6)

STRACK_SYMBOLS = ["ygz_hip_default_strack_params", "ygz_hip_stereo_track_search"]
STRACK_MAX_PROBLEMS, STRACK_MAX_SETS, STRACK_MAX_PAIRS, STRACK_TOPK = 64, 8, 262144, 8
STRACK_FRAME, STRACK_LOCAL = 0, 1
STRACK_SEARCHED, STRACK_SKIP, STRACK_BEHIND, STRACK_OUTSIDE, STRACK_RANGE, STRACK_ANGLE = range(6)
STRACK_MATCHED, STRACK_NO_CANDIDATE, STRACK_DISTANCE, STRACK_RATIO, STRACK_ORIENTATION = range(5)

SVO_SYMBOLS = ["ygz_hip_default_svo_params", "ygz_hip_stereo_odometry_slots"]
SVO_MAX_PAIRS = 1024
SVO_INT_OUTPUTS = ("match", "dist", "level", "reason", "outcome", "n_cand", "n_gated")
SVO_COUNTS = ("last_keypoints", "with_depth", "cur_keypoints", "matches", "searched", "overflowed", "removed_by_orientation", "retried")

SLM_SYMBOLS = ["ygz_hip_default_slm_params", "ygz_hip_stereo_local_map_slots"]
SLM_MAX_FRAMES, SLM_MAX_SETS, SLM_MAX_PAIRS = 1024, 64, 4194304
SLM_INT_OUTPUTS = ("match", "dist", "level", "reason", "outcome", "n_cand", "n_gated")
SLM_COUNTS = ("keypoints", "with_right_column", "prior_edges", "points", "searched", "overflowed", "new_matches", "edges")

SRK_SYMBOLS = ["ygz_hip_default_srk_params", "ygz_hip_stereo_ref_keyframe_slots"]
SRK_MAX_FRAMES, SRK_MAX_KEYFRAMES, SRK_MAX_SETS = 1024, 256, 64
SRK_COUNTS = ("keyframe_keypoints", "with_point", "keypoints", "with_right_column", "search_matches", "lost_claim", "removed_by_orientation", "edges")
SRK_MATCHED, SRK_NO_MATCH, SRK_LOST_CLAIM, SRK_ORIENTATION = 0, 1, 2, 4

SRL_SYMBOLS = ["ygz_hip_default_srl_params", "ygz_hip_stereo_relocalize_slots"]
SRL_MAX_FRAMES, SRL_MAX_PROBLEMS, SRL_MAX_KEYFRAMES, SRL_MAX_SETS, SRL_MAX_HYPOTHESIS_SETS = 256, 256, 256, 64, 76800
SRL_COUNTS = SRK_COUNTS + ("pnp_inliers", "final_inliers")
SRL_RELOCALISED, SRL_TOO_FEW_MATCHES, SRL_PNP_FAILED, SRL_TOO_FEW_INLIERS = range(4)

LMS_SYMBOLS = ["ygz_hip_default_lms_params", "ygz_hip_local_map_select"]
LMS_MAX_KEYFRAMES, LMS_MAX_COV, LMS_MAX_FRAMES, LMS_MAX_FEATURES = 4096, 32, 1024, 32768
LMS_OUTPUTS = ("votes", "ref", "n_voters", "n_local", "local_kf", "n_pt", "n_cut", "local_pt", "fr_prior")

MPA_SYMBOLS = ["ygz_hip_map_point_attributes", "ygz_hip_stereo_local_map_indexed"]
MPA_MAX_POINTS, MPA_MAX_LEVEL = 1048576, 30

RMAP_SYMBOLS = ["ygz_hip_map_create", "ygz_hip_map_destroy", "ygz_hip_map_info", "ygz_hip_map_upload", "ygz_hip_map_update", "ygz_hip_map_download",
                "ygz_hip_stereo_local_map_resident"]
RMAP_SELECT_OUTPUTS = ("votes", "ref", "n_voters", "n_local", "local_kf", "n_cut", "n_pt", "local_pt", "n_removed", "prior")
RMAP_DOWNLOAD = ("pw", "pt_desc", "pt_bad", "pt_has_desc", "kf_bad", "centre", "dmax", "normal", "state")

POPT_SYMBOLS = ["ygz_hip_default_pose_opt_params", "ygz_hip_optimize_pose_stereo"]
POPT_FAILED, POPT_CONVERGED, POPT_MAX_ITERATIONS, POPT_STALLED = range(4)
POPT_MAX_ROUNDS, POPT_MAX_STEPS = 8, 64

SUMMARY_FIELDS = 32

_lib = None


def load():
    """Load the in-tree HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libygz_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so).  If this library is mapped first it pulls in
        # /opt/rocm's copy, a later `import torch` maps the second one, and torch then reports "No HIP GPUs are available".  Mapped
        # after torch, libygz_hip.so binds to the runtime that is already there.  This harness (tests / bench.py, which use
        # torch.distributed) therefore imports torch first when it is installed; a C / C++ caller is not concerned.
        if "torch" not in sys.modules and os.environ.get("YGZ_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        _lib = C.CDLL(LIB_PATH)
        # C has no name mangling: a library built from an older header would still load.  Refuse it here.
        if not hasattr(_lib, "ygz_hip_abi_version") or _lib.ygz_hip_abi_version() != ABI_VERSION:
            got = _lib.ygz_hip_abi_version() if hasattr(_lib, "ygz_hip_abi_version") else None
            _lib = None
            raise ImportError("libygz_hip.so has ABI version %r, this binding was written for %d: rebuild (python -c 'import __graft_entry__ as g; g.build()')" % (got, ABI_VERSION))
        _lib.ygz_hip_error_string.restype = C.c_char_p
        _lib.ygz_hip_kf_row_bytes.restype = C.c_size_t
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def se3_chain(T_rel):
    """T[0] = identity, T[i] = T_rel[i] * T[i - 1] (host code of the library)"""
    T = np.ascontiguousarray(T_rel, np.float64).reshape(-1, 7)
    out = np.empty_like(T)
    rc = load().ygz_hip_se3_chain(_p(T, C.c_double), len(T), _p(out, C.c_double))
    if rc != OK:
        raise YgzHipError(rc, "se3_chain")
    return out


class PinnedArray:
    """numpy view of page-locked host memory (ygz_hip_pinned_alloc) -- asynchronous copies need it"""

    def __init__(self, shape, dtype):
        lib = load()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._ptr = C.c_void_p()
        lib.ygz_hip_pinned_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        rc = lib.ygz_hip_pinned_alloc(C.byref(self._ptr), max(self.nbytes, 64))
        if rc != OK:
            raise YgzHipError(rc, "ygz_hip_pinned_alloc")
        buf = (C.c_uint8 * max(self.nbytes, 64)).from_address(self._ptr.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self._ptr:
            self.array = None
            load().ygz_hip_pinned_free.argtypes = [C.c_void_p]
            load().ygz_hip_pinned_free(self._ptr)
            self._ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HipContext:
    """One ygz_hip_ctx: owns HBM frame slots on one GPU and one HIP stream."""

    def __init__(self, width=640, height=480, levels=3, max_frames=8, device=0, debug_maps=False, stream=None,
                 fast_threshold=15, cell_size=10, nms_tie_suppress=0, intrinsics=None):
        """intrinsics: (fx, fy, cx, cy) of the context's camera, or None for the defaults of ygz_hip_default_params"""
        self.lib = load()
        p = Params()
        self.lib.ygz_hip_default_params(C.byref(p))
        if intrinsics is not None:
            p.fx, p.fy, p.cx, p.cy = [float(v) for v in intrinsics]
        p.image_width, p.image_height, p.pyramid_levels = width, height, levels
        p.max_frames, p.debug_maps = max_frames, int(debug_maps)
        p.fast_threshold, p.cell_size, p.nms_tie_suppress = fast_threshold, cell_size, nms_tie_suppress
        self.params = p
        self._ctx = C.c_void_p()
        rc = self.lib.ygz_hip_create(C.byref(self._ctx), device, C.byref(p), C.c_void_p(stream))
        if rc != OK:
            self._ctx = C.c_void_p()
            raise YgzHipError(rc, "ygz_hip_create")
        self.width, self.height, self.levels, self.max_frames = width, height, levels, max_frames
        self.cells = self.lib.ygz_hip_max_keypoints(self._ctx)

    @classmethod
    def from_handle(cls, ptr, width, height, levels=3):
        """a NON-OWNING view of a context somebody else created (the lanes / BA context of the C++ offline driver): close() leaves it alone"""
        self = cls.__new__(cls)
        self.lib = load()
        p = Params()
        self.lib.ygz_hip_default_params(C.byref(p))
        p.image_width, p.image_height, p.pyramid_levels = width, height, levels
        self.params = p
        self._ctx = C.c_void_p(ptr)
        self._borrowed = True
        self.width, self.height, self.levels, self.max_frames = width, height, levels, 0
        self.cells = self.lib.ygz_hip_max_keypoints(self._ctx)
        return self

    def _chk(self, rc, what):
        if rc != OK:
            raise YgzHipError(rc, what, self.lib.ygz_hip_last_hip_error(self._ctx))

    def close(self):
        if self._ctx and not getattr(self, "_borrowed", False):
            self.lib.ygz_hip_destroy(self._ctx)
        self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._chk(self.lib.ygz_hip_synchronize(self._ctx), "synchronize")

    def join(self):
        """the context's stream waits for the stages pending on side streams; the host does not block"""
        self._chk(self.lib.ygz_hip_join(self._ctx), "join")

    def set_overlap(self, enable=True):
        self._chk(self.lib.ygz_hip_set_overlap(self._ctx, int(enable)), "set_overlap")

    def timer_begin(self):
        self._chk(self.lib.ygz_hip_timer_begin(self._ctx), "timer_begin")

    def timer_end(self):
        ms = C.c_float(0)
        self._chk(self.lib.ygz_hip_timer_end(self._ctx, C.byref(ms)), "timer_end")
        return ms.value

    def probe_begin(self, kernel, max_launches=4096):
        self._chk(self.lib.ygz_hip_probe_begin(self._ctx, kernel.encode(), max_launches), "probe_begin")

    def probe_end(self):
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.lib.ygz_hip_probe_end(self._ctx, C.byref(ms), C.byref(n)), "probe_end")
        return ms.value, n.value

    # ---- frames
    def upload_gray(self, slot, gray):
        gray = np.ascontiguousarray(gray, np.uint8)
        assert gray.shape == (self.height, self.width)
        self._chk(self.lib.ygz_hip_upload_gray(self._ctx, slot, _p(gray, C.c_uint8), self.width), "upload_gray")

    def upload_bgr(self, slot, bgr):
        bgr = np.ascontiguousarray(bgr, np.uint8)
        assert bgr.shape == (self.height, self.width, 3)
        self._chk(self.lib.ygz_hip_upload_bgr(self._ctx, slot, _p(bgr, C.c_uint8), self.width * 3), "upload_bgr")

    # ---- bulk traffic (arrays must be C-contiguous; wait=False needs page-locked memory, see PinnedArray)
    def upload_bgr_batch(self, slot_begin, bgr, wait=True):
        assert bgr.dtype == np.uint8 and bgr.flags["C_CONTIGUOUS"] and bgr.shape[1:] == (self.height, self.width, 3)
        self._chk(self.lib.ygz_hip_upload_bgr_batch(self._ctx, slot_begin, len(bgr), _p(bgr, C.c_uint8), int(wait)), "upload_bgr_batch")

    def upload_gray_batch(self, slot_begin, gray, wait=True):
        assert gray.dtype == np.uint8 and gray.flags["C_CONTIGUOUS"] and gray.shape[1:] == (self.height, self.width)
        self._chk(self.lib.ygz_hip_upload_gray_batch(self._ctx, slot_begin, len(gray), _p(gray, C.c_uint8), int(wait)), "upload_gray_batch")

    def get_keypoint_pixels_batch(self, slot_begin, n_slots, px=None, count=None, wait=True):
        px = np.empty((n_slots, self.cells, 2), np.float64) if px is None else px
        count = np.empty(n_slots, np.int32) if count is None else count
        self._chk(self.lib.ygz_hip_get_keypoint_pixels_batch(self._ctx, slot_begin, n_slots, _p(px, C.c_double), _p(count, C.c_int32), int(wait)),
                  "get_keypoint_pixels_batch")
        return px, count

    def get_keypoints_batch(self, slot_begin, n_slots, out=None, wait=True):
        if out is None:
            out = dict(px=np.empty((n_slots, self.cells, 2), np.float64), level=np.empty((n_slots, self.cells), np.int32),
                       score=np.empty((n_slots, self.cells), np.float32), angle=np.empty((n_slots, self.cells), np.float32),
                       desc=np.empty((n_slots, self.cells, 32), np.uint8), count=np.empty(n_slots, np.int32))
        f = lambda k, t: _p(out[k], t) if out.get(k) is not None else None
        soa = KptSoa(f("px", C.c_double), f("level", C.c_int32), f("score", C.c_float), f("angle", C.c_float), f("desc", C.c_uint8))
        self._chk(self.lib.ygz_hip_get_keypoints_batch(self._ctx, slot_begin, n_slots, C.byref(soa), _p(out["count"], C.c_int32), int(wait)),
                  "get_keypoints_batch")
        return out

    def set_keypoint_depths_batch(self, slot_begin, depth, has_mp, wait=True):
        assert depth.dtype == np.float64 and has_mp.dtype == np.uint8 and depth.shape[1] == self.cells and has_mp.shape == depth.shape
        self._chk(self.lib.ygz_hip_set_keypoint_depths_batch(self._ctx, slot_begin, len(depth), _p(depth, C.c_double), _p(has_mp, C.c_uint8),
                                                             int(wait)), "set_keypoint_depths_batch")

    def get_keypoint_counts(self, slot_begin, n_slots, out=None, wait=True):
        out = np.empty(n_slots, np.int32) if out is None else out
        self._chk(self.lib.ygz_hip_get_keypoint_counts(self._ctx, slot_begin, n_slots, _p(out, C.c_int32), int(wait)), "get_keypoint_counts")
        return out

    def upload_depth_batch(self, slot_begin, depth, scale=1.0, wait=True):
        """depth [n, dh, dw]: float32 / float64 metres, or uint16 with depth = value * scale"""
        assert depth.ndim == 3 and depth.flags["C_CONTIGUOUS"] and depth.dtype in (np.float32, np.uint16, np.float64)
        kind = {np.dtype(np.float32): 0, np.dtype(np.uint16): 1, np.dtype(np.float64): 2}[depth.dtype]
        self._chk(self.lib.ygz_hip_upload_depth_batch(self._ctx, slot_begin, len(depth), C.c_void_p(depth.ctypes.data), depth.shape[2], depth.shape[1],
                                                      kind, C.c_double(scale), int(wait)), "upload_depth_batch")

    def get_keypoint_depths(self, slot):
        d, m, n = np.empty(self.cells, np.float64), np.empty(self.cells, np.uint8), C.c_int(0)
        self._chk(self.lib.ygz_hip_get_keypoint_depths(self._ctx, slot, _p(d, C.c_double), _p(m, C.c_uint8), self.cells, C.byref(n)), "get_keypoint_depths")
        return d[:n.value].copy(), m[:n.value].copy()

    def keypoint_depths_from_image(self, slot_begin, n_slots):
        self._chk(self.lib.ygz_hip_keypoint_depths_from_image(self._ctx, slot_begin, n_slots), "keypoint_depths_from_image")

    # ---- stereo input
    def default_stereo_params(self, **fields):
        """ygz_stereo_params with the library's defaults, then the given fields"""
        p = StereoParams()
        stereo_argtypes(self.lib)
        self.lib.ygz_hip_default_stereo_params(C.byref(p))
        for k, v in fields.items():
            getattr(p, k)                   # AttributeError for a field the struct does not have
            setattr(p, k, v)
        return p

    def stereo_depths_slots(self, left_slots, right_slots, params=None, **fields):
        """the resident keypoints of the pairs (left_slots[q], right_slots[q]): dict of right_idx, u_right, depth, sad, status [n_pairs, cells]
        (-1 past a pair's left keypoints) and counts [n_pairs, 7]; with write_depths (the default) the left slots' keypoint depths are set"""
        p = params if params is not None else self.default_stereo_params(**fields)
        ls, rs = np.ascontiguousarray(left_slots, np.int32).reshape(-1), np.ascontiguousarray(right_slots, np.int32).reshape(-1)
        if len(ls) != len(rs):
            raise ValueError("left_slots and right_slots differ in length")
        n, c = len(ls), self.cells
        o = dict(right_idx=np.empty((n, c), np.int32), u_right=np.empty((n, c)), depth=np.empty((n, c)), sad=np.empty((n, c), np.int32),
                 status=np.empty((n, c), np.int32), counts=np.empty((n, STEREO_N_STATUS), np.int32))
        self._chk(self.lib.ygz_hip_stereo_depths_slots(self._ctx, n, _p(ls, C.c_int32), _p(rs, C.c_int32), C.byref(p), _p(o["right_idx"], C.c_int32),
                                                       _p(o["u_right"], C.c_double), _p(o["depth"], C.c_double), _p(o["sad"], C.c_int32),
                                                       _p(o["status"], C.c_int32), _p(o["counts"], C.c_int32)), "stereo_depths_slots")
        return o

    def _stereo_arrays(self, left_slot, right_slot, kl, kr, p):
        a = [np.ascontiguousarray(kl["px"], np.float64).reshape(-1, 2), np.ascontiguousarray(kl["level"], np.int32).reshape(-1),
             np.ascontiguousarray(kl["desc"], np.uint8).reshape(-1, 32)]
        b = [np.ascontiguousarray(kr["px"], np.float64).reshape(-1, 2), np.ascontiguousarray(kr["level"], np.int32).reshape(-1),
             np.ascontiguousarray(kr["desc"], np.uint8).reshape(-1, 32)]
        if not (len(a[0]) == len(a[1]) == len(a[2]) and len(b[0]) == len(b[1]) == len(b[2])):
            raise ValueError("px, level and desc of a keypoint list differ in length")
        f = lambda v, t: _p(v, t) if len(v) else None
        args = [self._ctx, int(left_slot), int(right_slot), f(a[0], C.c_double), f(a[1], C.c_int32), f(a[2], C.c_uint8), len(a[1]),
                f(b[0], C.c_double), f(b[1], C.c_int32), f(b[2], C.c_uint8), len(b[1]), C.byref(p)]
        return args, (a, b), len(a[1])

    def stereo_match(self, left_slot, right_slot, kl, kr, params=None, **fields):
        """the array form: keypoint lists kl, kr = dict(px [n, 2], level [n], desc [n, 32]) against the pictures of the two slots; dict of
        right_idx, u_right, depth, sad, status [nl] and counts [7].  Never writes depths."""
        p = params if params is not None else self.default_stereo_params(**fields)
        args, keep, n = self._stereo_arrays(left_slot, right_slot, kl, kr, p)
        o = dict(right_idx=np.empty(n, np.int32), u_right=np.empty(n), depth=np.empty(n), sad=np.empty(n, np.int32), status=np.empty(n, np.int32),
                 counts=np.empty(STEREO_N_STATUS, np.int32))
        self._chk(self.lib.ygz_hip_stereo_match(*args, _p(o["right_idx"], C.c_int32), _p(o["u_right"], C.c_double), _p(o["depth"], C.c_double),
                                                _p(o["sad"], C.c_int32), _p(o["status"], C.c_int32), _p(o["counts"], C.c_int32)), "stereo_match")
        return o

    def stereo_candidates(self, left_slot, right_slot, kl, kr, params=None, **fields):
        """the stages of the array form: best_idx, best_dist [nl] after the descriptor search (-1 without a candidate), n_cand [nl],
        sads [nl, 11] (-1 where the SAD search was not reached)"""
        p = params if params is not None else self.default_stereo_params(**fields)
        args, keep, n = self._stereo_arrays(left_slot, right_slot, kl, kr, p)
        o = dict(best_idx=np.empty(n, np.int32), best_dist=np.empty(n, np.int32), n_cand=np.empty(n, np.int32), sads=np.empty((n, STEREO_COLUMNS), np.int32))
        self._chk(self.lib.ygz_hip_stereo_candidates(*args, _p(o["best_idx"], C.c_int32), _p(o["best_dist"], C.c_int32), _p(o["n_cand"], C.c_int32),
                                                     _p(o["sads"], C.c_int32)), "stereo_candidates")
        return o

    # ---- stereo pose optimisation
    def default_pose_opt_params(self, **fields):
        """ygz_pose_opt_params with the library's defaults, then the given fields"""
        p = PoseOptParams()
        popt_argtypes(self.lib)
        self.lib.ygz_hip_default_pose_opt_params(C.byref(p))
        for k, v in fields.items():
            getattr(p, k)                   # AttributeError for a field the struct does not have
            setattr(p, k, v)
        return p

    def optimize_pose_stereo(self, frame_off, pw, obs, level, kind, poses, params=None, outputs=True, **fields):
        """ORB-SLAM2's PoseOptimization for the frames of the CSR list frame_off: pw, obs [n, 3], level, kind [n] (0 absent, 1 mono, 2 stereo),
        poses [n_frames, 7] (qx qy qz qw tx ty tz).  Dict of pose [n_frames, 7], outlier, chi2 [n], inliers, rounds_run [n_frames] and status,
        lm_iterations, cost_initial, cost_final, lambda [n_frames, 8]; outputs=False passes NULL for everything but the poses."""
        p = params if params is not None else self.default_pose_opt_params(**fields)
        popt_argtypes(self.lib)
        off = np.ascontiguousarray(frame_off, np.int32).reshape(-1)
        nf = len(off) - 1
        pw, obs = np.ascontiguousarray(pw, np.float64).reshape(-1, 3), np.ascontiguousarray(obs, np.float64).reshape(-1, 3)
        level, kind = np.ascontiguousarray(level, np.int32).reshape(-1), np.ascontiguousarray(kind, np.uint8).reshape(-1)
        n = len(level)
        if not (len(pw) == len(obs) == len(kind) == n):
            raise ValueError("pw, obs, level and kind differ in length")
        o = dict(pose=np.array(poses, np.float64).reshape(nf, 7))
        R = POPT_MAX_ROUNDS
        if outputs:
            o.update(outlier=np.zeros(n, np.uint8), chi2=np.zeros(n), inliers=np.zeros(nf, np.int32), rounds_run=np.zeros(nf, np.int32),
                     status=np.zeros((nf, R), np.int32), lm_iterations=np.zeros((nf, R), np.int32), cost_initial=np.zeros((nf, R)),
                     cost_final=np.zeros((nf, R)))
            o["lambda"] = np.zeros((nf, R))
        f = lambda key, t: _p(o[key], t) if outputs and o[key].size else None
        g = lambda v, t: _p(v, t) if len(v) else None
        self._chk(self.lib.ygz_hip_optimize_pose_stereo(
            self._ctx, nf, _p(off, C.c_int32), g(pw, C.c_double), g(obs, C.c_double), g(level, C.c_int32), g(kind, C.c_uint8), C.byref(p),
            _p(o["pose"], C.c_double) if nf else None, f("outlier", C.c_uint8), f("chi2", C.c_double), f("inliers", C.c_int32),
            f("rounds_run", C.c_int32), f("status", C.c_int32), f("lm_iterations", C.c_int32), f("cost_initial", C.c_double),
            f("cost_final", C.c_double), f("lambda", C.c_double)), "optimize_pose_stereo")
        return o

    # ---- stereo map-point creation
    def default_smap_params(self, **fields):
        """ygz_hip_default_smap_params, with the given fields overwritten"""
        smap_argtypes(self.lib)
        p = SmapParams()
        self.lib.ygz_hip_default_smap_params(C.byref(p))
        for k, v in fields.items():
            getattr(p, k)                   # AttributeError for a field the struct does not have
            setattr(p, k, v)
        return p

    def stereo_create_map_points(self, problems, K4, params=None, **fields):
        """ORB-SLAM2's CreateNewMapPoints with stereo for a list of problems, each a dict of T1, T2 [7], px1, px2 [n, 2], ur1, ur2, depth1,
        depth2 [n] (ur < 0: mono) and level1, level2 [n]; K4 = (fx, fy, cx, cy).  Dict of code, method [N], pos_world [N, 3] over the
        concatenated pairs, counts [n_problems, 2] (created, triangulated) and offsets [n_problems + 1]."""
        p = params if params is not None else self.default_smap_params(**fields)
        smap_argtypes(self.lib)
        arr = (SmapProblem * max(len(problems), 1))()
        keep, off = [], [0]
        for q, pb in enumerate(problems):
            T1, T2 = np.ascontiguousarray(pb["T1"], np.float64).reshape(7), np.ascontiguousarray(pb["T2"], np.float64).reshape(7)
            for k in range(7):
                arr[q].T1[k], arr[q].T2[k] = T1[k], T2[k]
            n = len(np.asarray(pb["ur1"]).reshape(-1))
            for name in ("px1", "px2", "ur1", "ur2", "depth1", "depth2", "level1", "level2"):
                t = np.int32 if name.startswith("level") else np.float64
                if pb.get(name) is None:
                    continue
                a = np.ascontiguousarray(pb[name], t).reshape(-1)
                if len(a) != n * (2 if name.startswith("px") else 1):
                    raise ValueError("problem %d: %s has the wrong length" % (q, name))
                keep.append(a)
                if n:
                    setattr(arr[q], name, _p(a, C.c_int32 if t is np.int32 else C.c_double))
            arr[q].n = n
            off.append(off[-1] + n)
        N = off[-1]
        m = max(N, 1)
        o = dict(code=np.zeros(m, np.int32), method=np.zeros(m, np.int32), pos_world=np.zeros((m, 3)),
                 counts=np.zeros((max(len(problems), 1), 2), np.int32), offsets=np.array(off, np.int32))
        k = np.ascontiguousarray(K4, np.float64).reshape(4)
        self._chk(self.lib.ygz_hip_stereo_create_map_points(self._ctx, len(problems), arr, _p(k, C.c_double), C.byref(p), _p(o["code"], C.c_int32),
                                                            _p(o["method"], C.c_int32), _p(o["pos_world"], C.c_double), _p(o["counts"], C.c_int32)),
                  "stereo_create_map_points")
        o["code"], o["method"], o["pos_world"], o["counts"] = o["code"][:N], o["method"][:N], o["pos_world"][:N], o["counts"][:len(problems)]
        return o

    def stereo_keyframe_points(self, T, px, depth, has_point, K4, params=None, **fields):
        """ORB-SLAM2's keyframe insertion for a stereo or RGB-D keyframe: the features with a depth, nearest first, the close ones and at least
        min_close of them un-projected into the world.  Dict of rank [n], selected [n], pos_world [n, 3], n_depth, n_close, n_selected."""
        p = params if params is not None else self.default_smap_params(**fields)
        smap_argtypes(self.lib)
        T = np.ascontiguousarray(T, np.float64).reshape(7)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        depth = np.ascontiguousarray(depth, np.float64).reshape(-1)
        has = np.ascontiguousarray(has_point, np.uint8).reshape(-1)
        n = len(depth)
        if not (len(px) == len(has) == n):
            raise ValueError("px, depth and has_point differ in length")
        m = max(n, 1)
        rank, sel, pos = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros((m, 3))
        nd, nc, ns = C.c_int(0), C.c_int(0), C.c_int(0)
        k = np.ascontiguousarray(K4, np.float64).reshape(4)
        g = lambda v, t: _p(v, t) if n else None
        self._chk(self.lib.ygz_hip_stereo_keyframe_points(self._ctx, _p(T, C.c_double), n, g(px, C.c_double), g(depth, C.c_double), g(has, C.c_uint8),
                                                          _p(k, C.c_double), C.byref(p), _p(rank, C.c_int32), _p(sel, C.c_uint8), _p(pos, C.c_double),
                                                          C.byref(nd), C.byref(nc), C.byref(ns)), "stereo_keyframe_points")
        return dict(rank=rank[:n], selected=sel[:n], pos_world=pos[:n], n_depth=nd.value, n_close=nc.value, n_selected=ns.value)

    # ---- local-map fusion search
    def default_lfuse_params(self, **fields):
        """ygz_hip_default_lfuse_params, with the given fields overwritten"""
        lfuse_argtypes(self.lib)
        p = LfuseParams()
        self.lib.ygz_hip_default_lfuse_params(C.byref(p))
        for k, v in fields.items():
            getattr(p, k)                   # AttributeError for a field the struct does not have
            setattr(p, k, v)
        return p

    def local_fuse_search(self, sets, problems, K4, params=None, **fields):
        """the search of ORB-SLAM2's Fuse for many target keyframes over shared point sets, one call.  sets: dicts of pw [n, 3], pt_desc
        [n, 32], pt_dmax [n], pt_normal [n, 3] (optional); problems: dicts of T [7], kp_px [m, 2], kp_level [m], kp_desc [m, 32], kp_ur [m]
        (optional, < 0: mono), kp_taken [m], pt_skip [n of its set] (optional) and set (default 0).  Dict of match, dist, pred_level,
        reason, n_gated [N] concatenated in problem order, counts [n_problems, 2] (matches, searched) and offsets [n_problems + 1]."""
        p = params if params is not None else self.default_lfuse_params(**fields)
        lfuse_argtypes(self.lib)
        keep = []

        def put(d, name, t, ct, n):
            a = d.get(name)
            if a is None:
                return C.POINTER(ct)()
            a = np.ascontiguousarray(a, t).reshape(-1)
            if len(a) != n:
                raise ValueError("%s has the wrong length" % name)
            keep.append(a)
            return _p(a, ct)
        sa = (LfusePoints * max(len(sets), 1))()
        for s, d in enumerate(sets):
            n = len(np.asarray(d["pt_dmax"]).reshape(-1))
            sa[s].pw, sa[s].pt_desc = put(d, "pw", np.float64, C.c_double, 3 * n), put(d, "pt_desc", np.uint8, C.c_uint8, 32 * n)
            sa[s].pt_dmax, sa[s].pt_normal = put(d, "pt_dmax", np.float64, C.c_double, n), put(d, "pt_normal", np.float64, C.c_double, 3 * n)
            sa[s].n_pt = n
        pa = (LfuseProblem * max(len(problems), 1))()
        off = [0]
        for q, d in enumerate(problems):
            T = np.ascontiguousarray(d["T"], np.float64).reshape(7)
            for k in range(7):
                pa[q].T[k] = T[k]
            m, st = len(np.asarray(d["kp_level"]).reshape(-1)), int(d.get("set", 0))
            n = int(sa[st].n_pt) if 0 <= st < len(sets) else 0
            pa[q].kp_px, pa[q].kp_level = put(d, "kp_px", np.float64, C.c_double, 2 * m), put(d, "kp_level", np.int32, C.c_int32, m)
            pa[q].kp_desc, pa[q].kp_ur = put(d, "kp_desc", np.uint8, C.c_uint8, 32 * m), put(d, "kp_ur", np.float64, C.c_double, m)
            pa[q].kp_taken, pa[q].pt_skip = put(d, "kp_taken", np.uint8, C.c_uint8, m), put(d, "pt_skip", np.uint8, C.c_uint8, n)
            pa[q].n_kp, pa[q].set = m, st
            off.append(off[-1] + n)
        N = off[-1]
        names = ("match", "dist", "pred_level", "reason", "n_gated")
        o = {k: np.full(max(N, 1), -7, np.int32) for k in names}
        counts = np.zeros((max(len(problems), 1), 2), np.int32)
        k4 = np.ascontiguousarray(K4, np.float64).reshape(4)
        self._chk(self.lib.ygz_hip_local_fuse_search(self._ctx, len(sets), sa, len(problems), pa, _p(k4, C.c_double), C.byref(p),
                                                     *[_p(o[k], C.c_int32) for k in names], _p(counts, C.c_int32)), "local_fuse_search")
        del keep
        o = {k: v[:N] for k, v in o.items()}
        o["counts"], o["offsets"] = counts[:len(problems)], np.array(off, np.int64)
        return o

    # ---- stereo tracking search
    def default_strack_params(self, **fields):
        """ygz_hip_default_strack_params, with the given fields overwritten"""
        strack_argtypes(self.lib)
        p = StrackParams()
        self.lib.ygz_hip_default_strack_params(C.byref(p))
        for k, v in fields.items():
            getattr(p, k)                   # AttributeError for a field the struct does not have
            setattr(p, k, v)
        return p

    def stereo_track_search(self, sets, problems, K4, params=None, **fields):
        """ORB-SLAM2's two tracking searches (frame to frame, local map) with the right-column gate, one call.  sets: dicts of pw [n, 3],
        pt_desc [n, 32] and pt_level [n], pt_angle [n] (optional) for FRAME or pt_dmax [n], pt_normal [n, 3] for LOCAL problems; problems:
        dicts of T [7], th, mode (0 FRAME, 1 LOCAL), direction, kp_px [m, 2], kp_level [m], kp_desc [m, 32], kp_ur [m] (optional, < 0:
        mono), kp_angle [m], kp_taken [m], pt_skip [n of its set] (optional) and set (default 0).  Dict of match, dist, level, reason,
        outcome, n_cand, n_gated [N], proj [N, 3], cand [N, 8] concatenated in problem order, counts [n_problems, 4] (matches, searched,
        overflowed, removed by orientation), rot [n_problems, 33] and offsets [n_problems + 1]."""
        p = params if params is not None else self.default_strack_params(**fields)
        strack_argtypes(self.lib)
        keep = []

        def put(d, name, t, ct, n):
            a = d.get(name)
            if a is None:
                return C.POINTER(ct)()
            a = np.ascontiguousarray(a, t).reshape(-1)
            if len(a) != n:
                raise ValueError("%s has the wrong length" % name)
            keep.append(a)
            return _p(a, ct)
        sa = (StrackPoints * max(len(sets), 1))()
        for s, d in enumerate(sets):
            n = len(np.asarray(d["pt_desc"]).reshape(-1)) // 32
            sa[s].pw, sa[s].pt_desc = put(d, "pw", np.float64, C.c_double, 3 * n), put(d, "pt_desc", np.uint8, C.c_uint8, 32 * n)
            sa[s].pt_level, sa[s].pt_angle = put(d, "pt_level", np.int32, C.c_int32, n), put(d, "pt_angle", np.float64, C.c_double, n)
            sa[s].pt_dmax, sa[s].pt_normal = put(d, "pt_dmax", np.float64, C.c_double, n), put(d, "pt_normal", np.float64, C.c_double, 3 * n)
            sa[s].n_pt = n
        pa = (StrackProblem * max(len(problems), 1))()
        off = [0]
        for q, d in enumerate(problems):
            T = np.ascontiguousarray(d["T"], np.float64).reshape(7)
            for k in range(7):
                pa[q].T[k] = T[k]
            m, st = len(np.asarray(d["kp_level"]).reshape(-1)), int(d.get("set", 0))
            n = int(sa[st].n_pt) if 0 <= st < len(sets) else 0
            pa[q].th, pa[q].mode, pa[q].direction = float(d["th"]), int(d.get("mode", 0)), int(d.get("direction", 0))
            pa[q].kp_px, pa[q].kp_level = put(d, "kp_px", np.float64, C.c_double, 2 * m), put(d, "kp_level", np.int32, C.c_int32, m)
            pa[q].kp_desc, pa[q].kp_ur = put(d, "kp_desc", np.uint8, C.c_uint8, 32 * m), put(d, "kp_ur", np.float64, C.c_double, m)
            pa[q].kp_angle = put(d, "kp_angle", np.float64, C.c_double, m)
            pa[q].kp_taken, pa[q].pt_skip = put(d, "kp_taken", np.uint8, C.c_uint8, m), put(d, "pt_skip", np.uint8, C.c_uint8, n)
            pa[q].n_kp, pa[q].set = m, st
            off.append(off[-1] + n)
        N, Q = off[-1], len(problems)
        names = ("match", "dist", "level", "reason", "outcome", "n_cand", "n_gated")
        o = {k: np.full(max(N, 1), -7, np.int32) for k in names}
        proj, cand = np.zeros((max(N, 1), 3), np.float64), np.full((max(N, 1), STRACK_TOPK), -7, np.int32)
        counts, rot = np.zeros((max(Q, 1), 4), np.int32), np.zeros((max(Q, 1), 33), np.int32)
        k4 = np.ascontiguousarray(K4, np.float64).reshape(4)
        self._chk(self.lib.ygz_hip_stereo_track_search(self._ctx, len(sets), sa, Q, pa, _p(k4, C.c_double), C.byref(p),
                                                       *[_p(o[k], C.c_int32) for k in names], _p(proj, C.c_double), _p(cand, C.c_int32),
                                                       _p(counts, C.c_int32), _p(rot, C.c_int32)), "stereo_track_search")
        del keep
        o = {k: v[:N] for k, v in o.items()}
        o["proj"], o["cand"], o["counts"], o["rot"], o["offsets"] = proj[:N], cand[:N], counts[:Q], rot[:Q], np.array(off, np.int64)
        return o

    # ---- stereo odometry on resident slots
    def default_svo_params(self, **fields):
        """ygz_hip_default_svo_params, with the given fields overwritten; a field of the embedded ygz_pose_opt_params is given as pose_<name>"""
        svo_argtypes(self.lib)
        p = SvoParams()
        self.lib.ygz_hip_default_svo_params(C.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p, k)
            getattr(tgt, name)              # AttributeError for a field the struct does not have
            setattr(tgt, name, v)
        return p

    def stereo_odometry_slots(self, last_slots, cur_slots, T_init=None, direction=None, params=None, outputs=True, **fields):
        """frame-to-frame stereo odometry for the resident pairs (last_slots[p], cur_slots[p]) in one call: the FRAME search with the
        right-column gate on the last frame's own depths, the claim walk, the orientation rule, the retry at twice the window and the u, v, uR
        pose optimisation.  T_init [n, 7] (None: identity), direction [n] (None: derived).  Dict of T_rel [n, 7], status [n], counts [n, 8],
        match, dist, level, reason, outcome, n_cand, n_gated [n, cells] by the last frame's keypoint, proj [n, cells, 3], rot [n, 33],
        outlier, chi2 [n, cells], inliers, rounds_run [n] and round_status, lm_iterations, cost_initial, cost_final, lambda [n, 8];
        outputs=False passes NULL for everything but T_rel and status."""
        p = params if params is not None else self.default_svo_params(**fields)
        svo_argtypes(self.lib)
        ls, cs = np.ascontiguousarray(last_slots, np.int32).reshape(-1), np.ascontiguousarray(cur_slots, np.int32).reshape(-1)
        if len(ls) != len(cs):
            raise ValueError("last_slots and cur_slots differ in length")
        n, c, R = len(ls), self.cells, POPT_MAX_ROUNDS
        T0 = None if T_init is None else np.ascontiguousarray(T_init, np.float64).reshape(n, 7)
        dr = None if direction is None else np.ascontiguousarray(direction, np.int32).reshape(n)
        m = max(n, 1)
        o = dict(T_rel=np.zeros((m, 7)), status=np.full(m, -7, np.int32))
        names = ("counts",) + SVO_INT_OUTPUTS + ("proj", "rot", "outlier", "chi2", "inliers", "rounds_run", "round_status", "lm_iterations",
                                                 "cost_initial", "cost_final", "lambda")
        if outputs:
            o.update(counts=np.full((m, 8), -7, np.int32), proj=np.zeros((m, c, 3)), rot=np.full((m, 33), -7, np.int32),
                     outlier=np.full((m, c), 7, np.uint8), chi2=np.zeros((m, c)), inliers=np.full(m, -7, np.int32),
                     rounds_run=np.full(m, -7, np.int32), round_status=np.full((m, R), -7, np.int32),
                     lm_iterations=np.full((m, R), -7, np.int32), cost_initial=np.zeros((m, R)), cost_final=np.zeros((m, R)))
            o["lambda"] = np.zeros((m, R))
            for k in SVO_INT_OUTPUTS:
                o[k] = np.full((m, c), -7, np.int32)
        types = {np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}
        f = lambda k: _p(o[k], types[o[k].dtype]) if k in o else None
        self._chk(self.lib.ygz_hip_stereo_odometry_slots(
            self._ctx, n, _p(ls, C.c_int32), _p(cs, C.c_int32), None if T0 is None else _p(T0, C.c_double),
            None if dr is None else _p(dr, C.c_int32), C.byref(p), f("T_rel"), f("status"), *[f(k) for k in names]), "stereo_odometry_slots")
        return {k: v[:n] for k, v in o.items()}

    # ---- stereo local-map tracking on resident slots
    def default_slm_params(self, **fields):
        """ygz_hip_default_slm_params, with the given fields overwritten; a field of the embedded ygz_pose_opt_params is given as pose_<name>"""
        slm_argtypes(self.lib)
        p = SlmParams()
        self.lib.ygz_hip_default_slm_params(C.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p, k)
            getattr(tgt, name)              # AttributeError for a field the struct does not have
            setattr(tgt, name, v)
        return p

    def stereo_local_map_slots(self, sets, slots, set_index, T, prior=None, params=None, outputs=True, **fields):
        """local-map tracking for the resident frames (slots[f], sets[set_index[f]]) in one call: the LOCAL search with the right-column gate,
        the claim walk and the u, v, uR pose optimisation on the prior and the new associations.  sets: dicts of pw [n, 3], pt_desc [n, 32],
        pt_dmax [n], pt_normal [n, 3] (an empty dict: a set of 0 points); T [n, 7]; prior [n, cells] (None: all free).  Dict of T_out [n, 7],
        status [n], counts [n, 8], kp_point, outlier, chi2 [n, cells], inliers, rounds_run [n], round_status, lm_iterations, cost_initial,
        cost_final, lambda [n, 8], match, dist, level, reason, outcome, n_cand, n_gated [N], proj [N, 3] concatenated in frame order and
        offsets [n + 1]; outputs=False passes NULL for everything but T_out and status."""
        p = params if params is not None else self.default_slm_params(**fields)
        slm_argtypes(self.lib)
        keep = []

        def put(d, name, t, ct, n):
            a = d.get(name)
            if a is None:
                return C.POINTER(ct)()
            a = np.ascontiguousarray(a, t).reshape(-1)
            if len(a) != n:
                raise ValueError("%s has the wrong length" % name)
            keep.append(a)
            return _p(a, ct)
        sa = (StrackPoints * max(len(sets), 1))()
        for s, d in enumerate(sets):
            n = len(np.asarray(d["pt_desc"]).reshape(-1)) // 32 if d.get("pt_desc") is not None else 0
            sa[s].pw, sa[s].pt_desc = put(d, "pw", np.float64, C.c_double, 3 * n), put(d, "pt_desc", np.uint8, C.c_uint8, 32 * n)
            sa[s].pt_dmax, sa[s].pt_normal = put(d, "pt_dmax", np.float64, C.c_double, n), put(d, "pt_normal", np.float64, C.c_double, 3 * n)
            sa[s].n_pt = n
        sl, st = np.ascontiguousarray(slots, np.int32).reshape(-1), np.ascontiguousarray(set_index, np.int32).reshape(-1)
        if len(sl) != len(st):
            raise ValueError("slots and set_index differ in length")
        n, c, R = len(sl), self.cells, POPT_MAX_ROUNDS
        T0 = np.ascontiguousarray(T, np.float64).reshape(n, 7)
        pr = None if prior is None else np.ascontiguousarray(prior, np.int32).reshape(n, c)
        off = [0]
        for f in range(n):
            off.append(off[-1] + (int(sa[int(st[f])].n_pt) if 0 <= st[f] < len(sets) else 0))
        N, m = off[-1], max(n, 1)
        o = dict(T_out=np.zeros((m, 7)), status=np.full(m, -7, np.int32))
        names = ("counts", "kp_point", "outlier", "chi2", "inliers", "rounds_run", "round_status", "lm_iterations", "cost_initial", "cost_final",
                 "lambda") + SLM_INT_OUTPUTS + ("proj",)
        if outputs:
            o.update(counts=np.full((m, 8), -7, np.int32), kp_point=np.full((m, c), -7, np.int32), outlier=np.full((m, c), 7, np.uint8),
                     chi2=np.zeros((m, c)), inliers=np.full(m, -7, np.int32), rounds_run=np.full(m, -7, np.int32),
                     round_status=np.full((m, R), -7, np.int32), lm_iterations=np.full((m, R), -7, np.int32), cost_initial=np.zeros((m, R)),
                     cost_final=np.zeros((m, R)), proj=np.zeros((max(N, 1), 3)))
            o["lambda"] = np.zeros((m, R))
            for k in SLM_INT_OUTPUTS:
                o[k] = np.full(max(N, 1), -7, np.int32)
        types = {np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}
        f_ = lambda k: _p(o[k], types[o[k].dtype]) if k in o else None
        self._chk(self.lib.ygz_hip_stereo_local_map_slots(
            self._ctx, len(sets), sa, n, _p(sl, C.c_int32), _p(st, C.c_int32), _p(T0, C.c_double), None if pr is None else _p(pr, C.c_int32),
            C.byref(p), f_("T_out"), f_("status"), *[f_(k) for k in names]), "stereo_local_map_slots")
        del keep
        per_point = SLM_INT_OUTPUTS + ("proj",)
        out = {k: (v[:N] if k in per_point else v[:n]) for k, v in o.items()}
        out["offsets"] = np.array(off, np.int64)
        return out

    # ---- stereo reference-keyframe tracking on resident slots
    def default_srk_params(self, **fields):
        """ygz_hip_default_srk_params, with the given fields overwritten; a field of the embedded ygz_pose_opt_params is given as pose_<name>"""
        srk_argtypes(self.lib)
        p = SrkParams()
        self.lib.ygz_hip_default_srk_params(C.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p, k)
            getattr(tgt, name)              # AttributeError for a field the struct does not have
            setattr(tgt, name, v)
        return p

    def stereo_ref_keyframe_slots(self, sets, kf_slot, kf_set, kf_point, slots, kf, T, params=None, outputs=True, **fields):
        """reference-keyframe tracking for the resident frames slots[f] against keyframe kf[f] (slot kf_slot[k], set sets[kf_set[k]], kf_point
        [n_kf, cells] the set index behind every keyframe keypoint or -1) in one call: BoW of every named slot, SearchByBoW, the claim, the
        rotation histogram and the u, v, uR pose optimisation from T [n, 7].  sets: dicts with pw [n_pt, 3] (an empty dict: a set of 0
        points; the other fields of a ygz_strack_points are not read).  Dict of T_out [n, 7], status [n], counts [n, 8], kp_point, prior,
        outlier, chi2 [n, cells], inliers, rounds_run [n], round_status, lm_iterations, cost_initial, cost_final, lambda [n, 8], match12,
        outcome [n, cells], rot [n, 33]; outputs=False passes NULL for everything but T_out, status and prior."""
        p = params if params is not None else self.default_srk_params(**fields)
        srk_argtypes(self.lib)
        keep = []
        sa = (StrackPoints * max(len(sets), 1))()
        for s, d in enumerate(sets):
            a = d.get("pw")
            a = np.zeros((0, 3)) if a is None else np.ascontiguousarray(a, np.float64).reshape(-1, 3)
            keep.append(a)
            sa[s].pw, sa[s].n_pt = (_p(a, C.c_double) if len(a) else C.POINTER(C.c_double)()), len(a)
        ks, kt = np.ascontiguousarray(kf_slot, np.int32).reshape(-1), np.ascontiguousarray(kf_set, np.int32).reshape(-1)
        sl, kk = np.ascontiguousarray(slots, np.int32).reshape(-1), np.ascontiguousarray(kf, np.int32).reshape(-1)
        if len(ks) != len(kt) or len(sl) != len(kk):
            raise ValueError("kf_slot and kf_set, or slots and kf, differ in length")
        n, c, R = len(sl), self.cells, POPT_MAX_ROUNDS
        kp = np.ascontiguousarray(kf_point, np.int32).reshape(len(ks), c)
        T0 = np.ascontiguousarray(T, np.float64).reshape(n, 7)
        m = max(n, 1)
        o = dict(T_out=np.zeros((m, 7)), status=np.full(m, -7, np.int32), prior=np.full((m, c), -7, np.int32))
        names = ("counts", "kp_point", "prior", "outlier", "chi2", "inliers", "rounds_run", "round_status", "lm_iterations", "cost_initial",
                 "cost_final", "lambda", "match12", "outcome", "rot")
        if outputs:
            o.update(counts=np.full((m, 8), -7, np.int32), kp_point=np.full((m, c), -7, np.int32), outlier=np.full((m, c), 7, np.uint8),
                     chi2=np.zeros((m, c)), inliers=np.full(m, -7, np.int32), rounds_run=np.full(m, -7, np.int32),
                     round_status=np.full((m, R), -7, np.int32), lm_iterations=np.full((m, R), -7, np.int32), cost_initial=np.zeros((m, R)),
                     cost_final=np.zeros((m, R)), match12=np.full((m, c), -7, np.int32), outcome=np.full((m, c), -7, np.int32),
                     rot=np.full((m, 33), -7, np.int32))
            o["lambda"] = np.zeros((m, R))
        types = {np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}
        f_ = lambda k: _p(o[k], types[o[k].dtype]) if k in o else None
        self._chk(self.lib.ygz_hip_stereo_ref_keyframe_slots(
            self._ctx, len(sets), sa, len(ks), _p(ks, C.c_int32), _p(kt, C.c_int32), _p(kp, C.c_int32), n, _p(sl, C.c_int32), _p(kk, C.c_int32),
            _p(T0, C.c_double), C.byref(p), f_("T_out"), f_("status"), *[f_(k) for k in names]), "stereo_ref_keyframe_slots")
        del keep
        return {k: v[:n] for k, v in o.items()}

    # ---- stereo relocalisation on resident slots
    def default_srl_params(self, **fields):
        """ygz_hip_default_srl_params, with the given fields overwritten; a field of the embedded ygz_pnp_params is given as pnp_<name>, one of
        the embedded ygz_pose_opt_params as pose_<name>"""
        srl_argtypes(self.lib)
        p = SrlParams()
        self.lib.ygz_hip_default_srl_params(C.byref(p))
        for k, v in fields.items():
            tgt, name = (p.pose, k[5:]) if k.startswith("pose_") else (p.pnp, k[4:]) if k.startswith("pnp_") else (p, k)
            getattr(tgt, name)              # AttributeError for a field the struct does not have
            setattr(tgt, name, v)
        return p

    def stereo_relocalize_slots(self, sets, kf_slot, kf_set, kf_point, slots, candidates, params=None, outputs=True, **fields):
        """relocalisation of the lost resident frames slots[f] against their ordered candidate keyframes candidates[f] (indices into kf_slot /
        kf_set / kf_point as in stereo_ref_keyframe_slots) in one call: BoW of every named slot, SearchByBoW, the claim, the rotation
        histogram, P3P RANSAC on the associations and the u, v, uR pose optimisation on its inliers; problem q is the q-th (frame, candidate)
        in the order given.  Dict of T_out [n, 7], best [n] (the winning problem or -1), cand_off [n + 1], and per problem status, T_pnp, T_opt,
        pnp_R, pnp_t, pnp_T_cw, pnp_success, pnp_n_inliers, pnp_best_sample, pnp_best_solution, pnp_n_hypotheses, counts [P, 10], inliers,
        rounds_run, round_status, lm_iterations, cost_initial, cost_final, lambda [P, 8], rot [P, 33], kp_point, pnp_inlier, prior, outlier,
        chi2, match12, outcome [P, cells], sets [P, max_iter, 3]; outputs=False passes NULL for everything but T_out, best, status, T_opt
        and prior."""
        p = params if params is not None else self.default_srl_params(**fields)
        srl_argtypes(self.lib)
        keep = []
        sa = (StrackPoints * max(len(sets), 1))()
        for s, d in enumerate(sets):
            a = d.get("pw")
            a = np.zeros((0, 3)) if a is None else np.ascontiguousarray(a, np.float64).reshape(-1, 3)
            keep.append(a)
            sa[s].pw, sa[s].n_pt = (_p(a, C.c_double) if len(a) else C.POINTER(C.c_double)()), len(a)
        ks, kt = np.ascontiguousarray(kf_slot, np.int32).reshape(-1), np.ascontiguousarray(kf_set, np.int32).reshape(-1)
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        if len(ks) != len(kt) or len(sl) != len(candidates):
            raise ValueError("kf_slot and kf_set, or slots and candidates, differ in length")
        off = np.concatenate([[0], np.cumsum([len(c) for c in candidates])]).astype(np.int32)
        ck = np.ascontiguousarray([k for c in candidates for k in c], np.int32).reshape(-1)
        n, P, c, R, it = len(sl), len(ck), self.cells, POPT_MAX_ROUNDS, max(int(p.pnp.max_iter), 1)
        kp = np.ascontiguousarray(kf_point, np.int32).reshape(len(ks), c)
        m, mp = max(n, 1), max(P, 1)
        o = dict(T_out=np.zeros((m, 7)), best=np.full(m, -7, np.int32), status=np.full(mp, -7, np.int32), T_opt=np.zeros((mp, 7)),
                 prior=np.full((mp, c), -7, np.int32))
        names = ("status", "T_pnp", "T_opt", "pnp", "counts", "inliers", "rounds_run", "round_status", "lm_iterations", "cost_initial",
                 "cost_final", "lambda", "rot", "kp_point", "pnp_inlier", "prior", "outlier", "chi2", "match12", "outcome", "sets")
        res = (PnpResult * mp)()
        if outputs:
            o.update(T_pnp=np.zeros((mp, 7)), counts=np.full((mp, 10), -7, np.int32), inliers=np.full(mp, -7, np.int32),
                     rounds_run=np.full(mp, -7, np.int32), round_status=np.full((mp, R), -7, np.int32),
                     lm_iterations=np.full((mp, R), -7, np.int32), cost_initial=np.zeros((mp, R)), cost_final=np.zeros((mp, R)),
                     rot=np.full((mp, 33), -7, np.int32), kp_point=np.full((mp, c), -7, np.int32), pnp_inlier=np.full((mp, c), 7, np.uint8),
                     outlier=np.full((mp, c), 7, np.uint8), chi2=np.zeros((mp, c)), match12=np.full((mp, c), -7, np.int32),
                     outcome=np.full((mp, c), -7, np.int32), sets=np.full((mp, it, 3), -7, np.int32))
            o["lambda"] = np.zeros((mp, R))
        types = {np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}
        f_ = lambda k: (res if outputs else None) if k == "pnp" else _p(o[k], types[o[k].dtype]) if k in o else None
        self._chk(self.lib.ygz_hip_stereo_relocalize_slots(
            self._ctx, len(sets), sa, len(ks), _p(ks, C.c_int32), _p(kt, C.c_int32), _p(kp, C.c_int32), n, _p(sl, C.c_int32), _p(off, C.c_int32),
            _p(ck, C.c_int32), C.byref(p), f_("T_out"), f_("best"), *[f_(k) for k in names]), "stereo_relocalize_slots")
        del keep
        out = {k: (v[:n] if k in ("T_out", "best") else v[:P]) for k, v in o.items()}
        if outputs:
            for k in ("R", "t", "T_cw"):
                out["pnp_" + k] = np.array([list(getattr(res[q], k)) for q in range(P)], np.float64).reshape(P, -1)
            for k in ("success", "n_inliers", "best_sample", "best_solution", "n_hypotheses"):
                out["pnp_" + k] = np.array([getattr(res[q], k) for q in range(P)], np.int32)
        out["cand_off"] = off
        return out

    # ---- keyframe store / device-built BA windows (configs[4])
    def stream_wait(self, signaler):
        self._chk(self.lib.ygz_hip_stream_wait(self._ctx, signaler._ctx), "stream_wait")

    def mark(self):
        self._chk(self.lib.ygz_hip_mark(self._ctx), "mark")

    def wait_mark(self, signaler):
        self._chk(self.lib.ygz_hip_wait_mark(self._ctx, signaler._ctx), "wait_mark")

    def kf_row_bytes(self, with_images=False):
        return int(self.lib.ygz_hip_kf_row_bytes(self._ctx, int(with_images)))

    def kf_store_create(self, n_keyframes, n_frames, max_windows, rows_ptr=None, rows_bytes=0, with_images=False):
        """with_images: the rows also hold the keyframes' pyramids (ba_build_windows(..., obs_mode=1) reads them)"""
        self._chk(self.lib.ygz_hip_kf_store_create(self._ctx, n_keyframes, n_frames, max_windows, C.c_void_p(rows_ptr) if rows_ptr else None,
                                                   C.c_size_t(rows_bytes), int(with_images)), "kf_store_create")

    def kf_store_info(self):
        rows, trel, rb, nk, nf = C.c_void_p(0), C.c_void_p(0), C.c_size_t(0), C.c_int(0), C.c_int(0)
        self._chk(self.lib.ygz_hip_kf_store_info(self._ctx, C.byref(rows), C.byref(rb), C.byref(trel), C.byref(nk), C.byref(nf)), "kf_store_info")
        return dict(rows=rows.value, row_bytes=rb.value, trel=trel.value, n_keyframes=nk.value, n_frames=nf.value)

    def kf_store_put(self, src, src_slots, kf_index):
        a = np.ascontiguousarray(src_slots, np.int32); b = np.ascontiguousarray(kf_index, np.int32)
        assert len(a) == len(b)
        self._chk(self.lib.ygz_hip_kf_store_put(self._ctx, src._ctx, len(a), _p(a, C.c_int32), _p(b, C.c_int32)), "kf_store_put")

    def kf_store_put_trel(self, src, first_pair, n_pairs, first_frame):
        self._chk(self.lib.ygz_hip_kf_store_put_trel(self._ctx, src._ctx, first_pair, n_pairs, first_frame), "kf_store_put_trel")

    def kf_store_set_trel(self, first_frame, T_rel):
        T = np.ascontiguousarray(T_rel, np.float64).reshape(-1, 7)
        self._chk(self.lib.ygz_hip_kf_store_set_trel(self._ctx, first_frame, len(T), _p(T, C.c_double)), "kf_store_set_trel")

    def kf_store_refresh(self):
        self._chk(self.lib.ygz_hip_kf_store_refresh(self._ctx), "kf_store_refresh")

    def ba_reserve_windows(self, window_begin, n_windows, K, max_points, huber_delta=5.991):
        self._chk(self.lib.ygz_hip_ba_reserve_windows(self._ctx, window_begin, n_windows, K, max_points, C.c_double(huber_delta)), "ba_reserve_windows")

    def ba_build_windows(self, window_begin, kf_index, kf_frame, n_kfs, obs_mode=0):
        """kf_index / kf_frame [n, K] (entries past n_kfs[i] ignored), n_kfs [n]; obs_mode 0: observations = good Hamming matches, 1: direct
        projection of the map points into the keyframes (FindCandidates + FindDirectProjection; the store must hold the images)"""
        a = np.ascontiguousarray(kf_index, np.int32); b = np.ascontiguousarray(kf_frame, np.int32); c = np.ascontiguousarray(n_kfs, np.int32)
        assert a.shape == b.shape and a.ndim == 2 and len(c) == len(a)
        self._chk(self.lib.ygz_hip_ba_build_windows(self._ctx, window_begin, len(a), _p(a, C.c_int32), _p(b, C.c_int32), _p(c, C.c_int32), int(obs_mode)),
                  "ba_build_windows")

    def ba_mark_outliers(self, window_begin, n_windows, chi2_threshold=5.991, disable=False):
        """BA.cpp:503-515 on the windows' current state (asynchronous, behind the resident LM)"""
        self._chk(self.lib.ygz_hip_ba_mark_outliers(self._ctx, window_begin, n_windows, C.c_double(chi2_threshold), int(disable)), "ba_mark_outliers")

    def ba_get_outlier_stats(self, window_begin, n_windows):
        """[n, 4]: edges tested, outliers, chi2 of the tested edges, chi2 of the inliers"""
        out = np.empty((n_windows, 4), np.float64)
        self._chk(self.lib.ygz_hip_ba_get_outlier_stats(self._ctx, window_begin, n_windows, _p(out, C.c_double)), "ba_get_outlier_stats")
        return out

    def ba_pack_states(self, window_begin, n_windows, row_doubles, dst_ptr=None, out=None, wait=True):
        """state rows into device memory at dst_ptr, or into (and returning) a host array [n_windows, row_doubles]"""
        if dst_ptr is not None:
            self._chk(self.lib.ygz_hip_ba_pack_states(self._ctx, window_begin, n_windows, C.c_void_p(dst_ptr), C.c_size_t(row_doubles), 1, int(wait)), "ba_pack_states")
            return None
        out = np.empty((n_windows, row_doubles), np.float64) if out is None else out
        self._chk(self.lib.ygz_hip_ba_pack_states(self._ctx, window_begin, n_windows, C.c_void_p(out.ctypes.data), C.c_size_t(row_doubles), 0, int(wait)), "ba_pack_states")
        return out

    def ba_get_stats(self, window_begin, n_windows, want_stats=True):
        """(statistics of the last resident LM run per window, dims [n, 4] = poses, points, edges, free poses)"""
        st = (BaStats * n_windows)()
        dims = np.empty((n_windows, 4), np.int32)
        self._chk(self.lib.ygz_hip_ba_get_stats(self._ctx, window_begin, n_windows, st if want_stats else None, _p(dims, C.c_int32)), "ba_get_stats")
        return (list(st) if want_stats else None), dims

    def ba_lm_iterations(self, window_begin, n_windows):
        """iterations of the last resident LM run per window WITHOUT raising: < 0 = the team timed out at a barrier (or no run yet)"""
        st = (BaStats * n_windows)()
        rc = self.lib.ygz_hip_ba_get_stats(self._ctx, window_begin, n_windows, st, None)
        if rc not in (OK, E_HIP, E_STATE):
            self._chk(rc, "ba_get_stats")
        return [s.iterations for s in st]

    def track_get_summary(self, out=None, wait=True):
        if out is None:
            out = np.empty((self.max_frames, SUMMARY_FIELDS), np.float64)
        n = C.c_int(0)
        self._chk(self.lib.ygz_hip_track_get_summary(self._ctx, _p(out, C.c_double), len(out), C.byref(n), int(wait)), "track_get_summary")
        return out[:n.value]

    def build_pyramid(self, slot_begin=0, n_slots=1, from_bgr=False):
        self._chk(self.lib.ygz_hip_build_pyramid(self._ctx, slot_begin, n_slots, int(from_bgr)), "build_pyramid")

    # ---- lens undistortion
    def default_undistort_params(self):
        p = UndistortParams()
        undistort_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_default_undistort_params(self._ctx, C.byref(p)), "default_undistort_params")
        return p

    def set_undistortion(self, drop=False, **fields):
        """builds the map from the defaults (the context's camera, no distortion, border 0) with the given fields of ygz_undistort_params
        replaced; drop=True removes it"""
        undistort_argtypes(self.lib)
        if drop:
            self._chk(self.lib.ygz_hip_set_undistortion(self._ctx, None), "set_undistortion")
            return None
        p = self.default_undistort_params()
        for k, v in fields.items():
            setattr(p, k, v)
        self._chk(self.lib.ygz_hip_set_undistortion(self._ctx, C.byref(p)), "set_undistortion")
        return p

    def undistort_map(self):
        """(qx, qy) [h, w] int32: source positions in 1/32 pixel, UNDISTORT_OUTSIDE in both where the picture has nothing"""
        undistort_argtypes(self.lib)
        qx, qy = np.empty((self.height, self.width), np.int32), np.empty((self.height, self.width), np.int32)
        self._chk(self.lib.ygz_hip_undistort_map(self._ctx, _p(qx, C.c_int32), _p(qy, C.c_int32)), "undistort_map")
        return qx, qy

    def build_pyramid_undistorted(self, slot_begin=0, n_slots=1, from_bgr=False):
        self._chk(self.lib.ygz_hip_build_pyramid_undistorted(self._ctx, slot_begin, n_slots, int(from_bgr)), "build_pyramid_undistorted")

    # ---- stereo rectification
    def default_rectify_params(self):
        p = RectifyParams()
        rectify_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_default_rectify_params(self._ctx, C.byref(p)), "default_rectify_params")
        return p

    def set_rectification(self, camera, R=None, drop=False, **lens):
        """builds the map and the tile table of rig camera `camera` from the defaults (the context's camera, no distortion, border 0, R = I)
        with R [3, 3] and the given fields of the lens replaced; drop=True removes them"""
        rectify_argtypes(self.lib)
        if drop:
            self._chk(self.lib.ygz_hip_set_rectification(self._ctx, camera, None), "set_rectification")
            return None
        p = self.default_rectify_params()
        for k, v in lens.items():
            setattr(p.lens, k, v)
        if R is not None:
            p.R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
        self._chk(self.lib.ygz_hip_set_rectification(self._ctx, camera, C.byref(p)), "set_rectification")
        return p

    def rectify_map(self, camera):
        """(qx, qy) [h, w] int32 of a rig camera: source positions in 1/32 pixel, UNDISTORT_OUTSIDE in both where the picture has nothing"""
        rectify_argtypes(self.lib)
        qx, qy = np.empty((self.height, self.width), np.int32), np.empty((self.height, self.width), np.int32)
        self._chk(self.lib.ygz_hip_rectify_map(self._ctx, camera, _p(qx, C.c_int32), _p(qy, C.c_int32)), "rectify_map")
        return qx, qy

    def build_pyramid_rectified(self, camera_of_slot, slot_begin=0, from_bgr=False):
        """level 0 of slot slot_begin + i = its upload through the map of rig camera camera_of_slot[i]"""
        rectify_argtypes(self.lib)
        cams = np.ascontiguousarray(camera_of_slot, np.uint8).reshape(-1)
        self._chk(self.lib.ygz_hip_build_pyramid_rectified(self._ctx, slot_begin, len(cams), int(from_bgr), _p(cams, C.c_uint8)), "build_pyramid_rectified")

    def level_size(self, level):
        w, h = C.c_int(0), C.c_int(0)
        self._chk(self.lib.ygz_hip_level_size(self._ctx, level, C.byref(w), C.byref(h)), "level_size")
        return w.value, h.value

    def download_level(self, slot, level):
        w, h = self.level_size(level)
        out = np.empty((h, w), np.uint8)
        self._chk(self.lib.ygz_hip_download_level(self._ctx, slot, level, _p(out, C.c_uint8)), "download_level")
        return out

    # ---- extractor
    def download_framed_level(self, slot, level):
        """the tracker's working image of a level (24-pixel reflect-101 frame), or None when the slot has no current framed copy"""
        w, h = self.level_size(level)
        out = np.empty((h + 48, w + 48), np.uint8)
        rc = self.lib.ygz_hip_download_framed_level(self._ctx, slot, level, _p(out, C.c_uint8))
        if rc == E_STATE:
            return None
        self._chk(rc, "download_framed_level")
        return out

    def detect(self, slot_begin=0, n_slots=1, occupied=None):
        occ = None
        if occupied is not None:
            occupied = np.ascontiguousarray(occupied, np.uint8).reshape(n_slots, self.cells)
            occ = _p(occupied, C.c_uint8)
        self._chk(self.lib.ygz_hip_detect(self._ctx, slot_begin, n_slots, occ), "detect")

    def keypoint_count(self, slot):
        n = C.c_int(0)
        self._chk(self.lib.ygz_hip_keypoint_count(self._ctx, slot, C.byref(n)), "keypoint_count")
        return n.value

    def get_keypoints(self, slot):
        cap = self.cells
        px = np.empty((cap, 2), np.float64)
        level = np.empty(cap, np.int32)
        score = np.empty(cap, np.float32)
        angle = np.empty(cap, np.float32)
        desc = np.empty((cap, 32), np.uint8)
        soa = KptSoa(_p(px, C.c_double), _p(level, C.c_int32), _p(score, C.c_float), _p(angle, C.c_float), _p(desc, C.c_uint8))
        n = C.c_int(0)
        self._chk(self.lib.ygz_hip_get_keypoints(self._ctx, slot, C.byref(soa), cap, C.byref(n)), "get_keypoints")
        n = n.value
        return dict(px=px[:n].copy(), level=level[:n].copy(), score=score[:n].copy(), angle=angle[:n].copy(), desc=desc[:n].copy())

    def describe(self, slot, px, level):
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        level = np.ascontiguousarray(level, np.int32)
        self._chk(self.lib.ygz_hip_describe(self._ctx, slot, _p(px, C.c_double), _p(level, C.c_int32), len(level)), "describe")

    def describe_given_angle(self, slot, px, level, angle):
        """ComputeOrbDescriptor alone with the caller's angles (degrees) -- what FeatureDetector::ComputeDescriptor(Feature*) calls"""
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        level = np.ascontiguousarray(level, np.int32)
        angle = np.ascontiguousarray(angle, np.float32)
        self._chk(self.lib.ygz_hip_describe_given_angle(self._ctx, slot, _p(px, C.c_double), _p(level, C.c_int32), _p(angle, C.c_float), len(level)),
                  "describe_given_angle")

    def get_device(self):
        dev, cus = C.c_int(-1), C.c_int(0)
        self._chk(self.lib.ygz_hip_get_device(self._ctx, C.byref(dev), C.byref(cus)), "get_device")
        return dev.value, cus.value

    def get_fast_maps(self, slot, level):
        w, h = self.level_size(level)
        score = np.empty((h, w), np.uint8)
        nms = np.empty((h, w), np.uint8)
        self._chk(self.lib.ygz_hip_get_fast_maps(self._ctx, slot, level, _p(score, C.c_uint8), _p(nms, C.c_uint8)), "get_fast_maps")
        return score, nms

    # ---- matcher
    def match_slots(self, query_slots, train_slots, cross_check=1):
        q = np.ascontiguousarray(query_slots, np.int32)
        t = np.ascontiguousarray(train_slots, np.int32)
        self._chk(self.lib.ygz_hip_match_slots(self._ctx, _p(q, C.c_int32), _p(t, C.c_int32), len(q), cross_check), "match_slots")

    def match_slots_again(self, cross_check=1):
        self._chk(self.lib.ygz_hip_match_slots_again(self._ctx, cross_check), "match_slots_again")

    def get_matches(self, pair):
        idx = np.empty(self.cells, np.int32)
        dist = np.empty(self.cells, np.int32)
        n = C.c_int(0)
        self._chk(self.lib.ygz_hip_get_matches(self._ctx, pair, _p(idx, C.c_int32), _p(dist, C.c_int32), self.cells, C.byref(n)), "get_matches")
        return idx[:n.value].copy(), dist[:n.value].copy()

    def hamming_match(self, q, t, cross_check=1, want_second=False):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx = np.empty(len(q), np.int32)
        dist = np.empty(len(q), np.int32)
        d2 = np.empty(len(q), np.int32) if want_second else None
        self._chk(self.lib.ygz_hip_hamming_match(self._ctx, _p(q, C.c_uint8), len(q), _p(t, C.c_uint8), len(t), cross_check,
                                                 _p(idx, C.c_int32), _p(dist, C.c_int32),
                                                 _p(d2, C.c_int32) if want_second else None), "hamming_match")
        return (idx, dist, d2) if want_second else (idx, dist)

    # ---- M3 / M6 filters
    def match_postfilter(self, min_floor=20.0, min_ceil=50.0, factor=3.0):
        self._chk(self.lib.ygz_hip_match_postfilter(self._ctx, C.c_double(min_floor), C.c_double(min_ceil), C.c_double(factor)), "match_postfilter")

    def get_good_matches(self, pair):
        good = np.zeros(self.cells, np.uint8)
        n, ng, md = C.c_int(0), C.c_int(0), C.c_double(0)
        self._chk(self.lib.ygz_hip_get_good_matches(self._ctx, pair, _p(good, C.c_uint8), self.cells, C.byref(n), C.byref(ng), C.byref(md)),
                  "get_good_matches")
        return good[:n.value].astype(bool), ng.value, md.value

    def match_postfilter_host(self, train_idx, dist, min_floor=20.0, min_ceil=50.0, factor=3.0):
        ti = np.ascontiguousarray(train_idx, np.int32); di = np.ascontiguousarray(dist, np.int32)
        good = np.zeros(max(len(ti), 1), np.uint8)
        ng, md = C.c_int(0), C.c_double(0)
        self._chk(self.lib.ygz_hip_match_postfilter_host(self._ctx, _p(ti, C.c_int32), _p(di, C.c_int32), len(ti), C.c_double(min_floor),
                                                         C.c_double(min_ceil), C.c_double(factor), _p(good, C.c_uint8), C.byref(ng), C.byref(md)),
                  "match_postfilter_host")
        return good[:len(ti)].astype(bool), ng.value, md.value

    def match_sets(self, descs, pair_q, pair_t, cross_check=1, good_filter=True, min_floor=20.0, min_ceil=50.0, factor=3.0):
        """M1-M3 over host descriptor sets in ONE call: descs = list of [n_s, 32] uint8 arrays; returns per pair (rows of the query set)
        train_idx, dist and -- with good_filter -- the kept flags, their count and the clamped minimum distance"""
        ds = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in descs]
        n_sets, n_pairs = len(ds), len(pair_q)
        ptrs = (C.POINTER(C.c_uint8) * n_sets)(*[_p(d, C.c_uint8) for d in ds])
        cnt = np.array([len(d) for d in ds], np.int32)
        pq = np.ascontiguousarray(pair_q, np.int32); pt = np.ascontiguousarray(pair_t, np.int32)
        idx = np.empty((n_pairs, self.cells), np.int32); dist = np.empty((n_pairs, self.cells), np.int32)
        good = np.zeros((n_pairs, self.cells), np.uint8) if good_filter else None
        ng = np.zeros(n_pairs, np.int32); md = np.zeros(n_pairs, np.float64)
        self.lib.ygz_hip_match_sets.argtypes = None
        self._chk(self.lib.ygz_hip_match_sets(self._ctx, n_sets, ptrs, _p(cnt, C.c_int32), n_pairs, _p(pq, C.c_int32), _p(pt, C.c_int32), cross_check,
                                              _p(idx, C.c_int32), _p(dist, C.c_int32), _p(good, C.c_uint8) if good_filter else None,
                                              _p(ng, C.c_int32) if good_filter else None, _p(md, C.c_double) if good_filter else None,
                                              C.c_double(min_floor), C.c_double(min_ceil), C.c_double(factor)), "match_sets")
        out = []
        for p in range(n_pairs):
            n = int(cnt[pq[p]])
            r = dict(idx=idx[p, :n], dist=dist[p, :n])
            if good_filter:
                r.update(good=good[p, :n].astype(bool), n_good=int(ng[p]), min_dis=float(md[p]))
            out.append(r)
        return out

    def check_frame_descriptors(self, slot1, slot2, idx1, idx2, init_low=30, init_high=80, ratio=3.0):
        i1 = np.ascontiguousarray(idx1, np.int32); i2 = np.ascontiguousarray(idx2, np.int32)
        n = len(i1)
        dist = np.zeros(max(n, 1), np.int32); keep = np.zeros(max(n, 1), np.uint8)
        ng, best = C.c_int(0), C.c_int(0)
        self._chk(self.lib.ygz_hip_check_frame_descriptors(self._ctx, slot1, slot2, _p(i1, C.c_int32), _p(i2, C.c_int32), n, init_low, init_high,
                                                           C.c_float(ratio), _p(dist, C.c_int32), _p(keep, C.c_uint8), C.byref(ng), C.byref(best)),
                  "check_frame_descriptors")
        return dist[:n].copy(), keep[:n].astype(bool), ng.value, best.value

    def check_descriptor_pairs(self, desc1, desc2, init_low=30, init_high=80, ratio=3.0):
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        n = len(d1)
        dist = np.zeros(max(n, 1), np.int32); keep = np.zeros(max(n, 1), np.uint8)
        ng, best = C.c_int(0), C.c_int(0)
        self._chk(self.lib.ygz_hip_check_descriptor_pairs(self._ctx, _p(d1, C.c_uint8), _p(d2, C.c_uint8), n, init_low, init_high, C.c_float(ratio),
                                                          _p(dist, C.c_int32), _p(keep, C.c_uint8), C.byref(ng), C.byref(best)),
                  "check_descriptor_pairs")
        return dist[:n].copy(), keep[:n].astype(bool), ng.value, best.value

    # ---- alignment
    def sparse_align_residuals(self, ref_slot, cur_slot, T_cur_from_ref, px, depth, has_mp, level):
        """one SparseImgAlign::computeResiduals(model, linearize = true) at `level`: (chi2 float sum, n_meas, H [6][6], Jres [6])"""
        T = np.ascontiguousarray(T_cur_from_ref, np.float64)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2); depth = np.ascontiguousarray(depth, np.float64)
        has_mp = np.ascontiguousarray(has_mp, np.uint8)
        chi2, nm = C.c_double(0), C.c_int(0)
        H, J = np.zeros(36), np.zeros(6)
        self.lib.ygz_hip_sparse_align_residuals.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                            C.POINTER(C.c_uint8), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                                            C.POINTER(C.c_double), C.POINTER(C.c_double)]
        self._chk(self.lib.ygz_hip_sparse_align_residuals(self._ctx, int(ref_slot), int(cur_slot), _p(T, C.c_double), _p(px, C.c_double), _p(depth, C.c_double),
                                                          _p(has_mp, C.c_uint8), len(depth), int(level), C.byref(chi2), C.byref(nm), _p(H, C.c_double),
                                                          _p(J, C.c_double)), "sparse_align_residuals")
        return chi2.value, nm.value, H.reshape(6, 6), J

    def find_direct_projection_mp(self, cur_slot, T_cur, kf_slots, kf_T, cand_kf, pos_world, px_ref, level_ref, px_in=None):
        """Matcher::FindDirectProjection, MapPoint overload, per candidate over several reference keyframes in one launch.
        Returns dict(in_view, px_proj, ok, px, level); px_in given: no FindCandidates projection, every candidate evaluated."""
        T_cur = np.ascontiguousarray(T_cur, np.float64); kf_slots = np.ascontiguousarray(kf_slots, np.int32)
        kf_T = np.ascontiguousarray(kf_T, np.float64).reshape(-1, 7); cand_kf = np.ascontiguousarray(cand_kf, np.int32)
        pos_world = np.ascontiguousarray(pos_world, np.float64).reshape(-1, 3); px_ref = np.ascontiguousarray(px_ref, np.float64).reshape(-1, 2)
        level_ref = np.ascontiguousarray(level_ref, np.int32)
        n = len(cand_kf)
        vis = np.zeros(n, np.uint8); proj = np.zeros((n, 2)); ok = np.zeros(n, np.uint8); px = np.zeros((n, 2)); sl = np.zeros(n, np.int32)
        pin = None
        if px_in is not None:
            pin = np.ascontiguousarray(px_in, np.float64).reshape(-1, 2)
        self.lib.ygz_hip_find_direct_projection_mp.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                               C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                                               C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_uint8),
                                                               C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_find_direct_projection_mp(self._ctx, int(cur_slot), _p(T_cur, C.c_double), len(kf_slots), _p(kf_slots, C.c_int32),
                                                             _p(kf_T, C.c_double), n, _p(cand_kf, C.c_int32), _p(pos_world, C.c_double), _p(px_ref, C.c_double),
                                                             _p(level_ref, C.c_int32), None if pin is None else _p(pin, C.c_double), _p(vis, C.c_uint8),
                                                             _p(proj, C.c_double), _p(ok, C.c_uint8), _p(px, C.c_double), _p(sl, C.c_int32)),
                  "find_direct_projection_mp")
        return dict(in_view=vis.astype(bool), px_proj=proj, ok=ok.astype(bool), px=px, level=sl)

    def find_direct_projection_mp_begin(self, cur_slot, T_cur, kf_slots, kf_T, cand_kf, pos_world, px_ref, level_ref):
        """first half of find_direct_projection_mp (px_in = None form): queued, not waited for; returns the candidate count for ..._end"""
        T_cur = np.ascontiguousarray(T_cur, np.float64); kf_slots = np.ascontiguousarray(kf_slots, np.int32)
        kf_T = np.ascontiguousarray(kf_T, np.float64).reshape(-1, 7); cand_kf = np.ascontiguousarray(cand_kf, np.int32)
        pos_world = np.ascontiguousarray(pos_world, np.float64).reshape(-1, 3); px_ref = np.ascontiguousarray(px_ref, np.float64).reshape(-1, 2)
        level_ref = np.ascontiguousarray(level_ref, np.int32)
        self.lib.ygz_hip_find_direct_projection_mp_begin.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                                     C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_find_direct_projection_mp_begin(self._ctx, int(cur_slot), _p(T_cur, C.c_double), len(kf_slots), _p(kf_slots, C.c_int32),
                                                                   _p(kf_T, C.c_double), len(cand_kf), _p(cand_kf, C.c_int32), _p(pos_world, C.c_double),
                                                                   _p(px_ref, C.c_double), _p(level_ref, C.c_int32)), "find_direct_projection_mp_begin")
        return len(cand_kf)

    def find_direct_projection_mp_end(self, n):
        vis = np.zeros(n, np.uint8); proj = np.zeros((n, 2)); ok = np.zeros(n, np.uint8); px = np.zeros((n, 2)); sl = np.zeros(n, np.int32)
        self.lib.ygz_hip_find_direct_projection_mp_end.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_uint8),
                                                                   C.POINTER(C.c_double), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_find_direct_projection_mp_end(self._ctx, int(n), _p(vis, C.c_uint8), _p(proj, C.c_double), _p(ok, C.c_uint8),
                                                                 _p(px, C.c_double), _p(sl, C.c_int32)), "find_direct_projection_mp_end")
        return dict(in_view=vis.astype(bool), px_proj=proj, ok=ok.astype(bool), px=px, level=sl)

    def find_direct_projection(self, ref_slot, T_ref, cur_slot, T_cur, px_ref, depth_ref, level_ref, px_cur):
        pair = AlignPair(ref_slot, cur_slot, (C.c_double * 7)(*T_ref), (C.c_double * 7)(*T_cur))
        px_ref = np.ascontiguousarray(px_ref, np.float64).reshape(-1, 2)
        depth_ref = np.ascontiguousarray(depth_ref, np.float64)
        level_ref = np.ascontiguousarray(level_ref, np.int32)
        px_cur = np.ascontiguousarray(px_cur, np.float64).reshape(-1, 2).copy()
        n = len(depth_ref)
        sl = np.empty(n, np.int32)
        ok = np.empty(n, np.uint8)
        self._chk(self.lib.ygz_hip_find_direct_projection(self._ctx, C.byref(pair), _p(px_ref, C.c_double), _p(depth_ref, C.c_double),
                                                          _p(level_ref, C.c_int32), _p(px_cur, C.c_double), _p(sl, C.c_int32),
                                                          _p(ok, C.c_uint8), n), "find_direct_projection")
        return ok.astype(bool), px_cur, sl

    def track_local_map(self, cur_slot, T_cur, kf_slot, kf_T, pos_world, point_bad, cand_point, cand_kf, cand_px_ref, cand_level):
        """LocalMapping::FindCandidates + ProjectMapPoints (LocalMapping.cpp:47-120) -> n, in_view, px_proj, match_cand, px_match, level"""
        pw = np.ascontiguousarray(pos_world, np.float64).reshape(-1, 3)
        P = pw.shape[0]
        bad = None if point_bad is None else np.ascontiguousarray(point_bad, np.uint8)
        ks = np.ascontiguousarray(kf_slot, np.int32); kT = np.ascontiguousarray(kf_T, np.float64).reshape(-1, 7)
        cp = np.ascontiguousarray(cand_point, np.int32); ck = np.ascontiguousarray(cand_kf, np.int32)
        cl = np.ascontiguousarray(cand_level, np.int32); cx = np.ascontiguousarray(cand_px_ref, np.float64).reshape(-1, 2)
        m = LocalMap(P, _p(pw, C.c_double), _p(bad, C.c_uint8) if bad is not None else None, len(ks), _p(ks, C.c_int32), _p(kT, C.c_double),
                     len(cp), _p(cp, C.c_int32), _p(ck, C.c_int32), _p(cl, C.c_int32), _p(cx, C.c_double))
        in_view = np.zeros(P, np.uint8); px_proj = np.zeros((P, 2)); match = np.full(P, -1, np.int32)
        px_match = np.zeros((P, 2)); lvl = np.zeros(P, np.int32)
        n = C.c_int32(0)
        T = (C.c_double * 7)(*[float(x) for x in T_cur])
        self.lib.ygz_hip_track_local_map.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(LocalMap), C.POINTER(C.c_uint8),
                                                     C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                                     C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_track_local_map(self._ctx, int(cur_slot), T, C.byref(m), _p(in_view, C.c_uint8), _p(px_proj, C.c_double),
                                                   _p(match, C.c_int32), _p(px_match, C.c_double), _p(lvl, C.c_int32), C.byref(n)), "track_local_map")
        return int(n.value), in_view, px_proj, match, px_match, lvl

    def align2d(self, cur_slot, level, pwb, uv, n_iter=10):
        pwb = np.ascontiguousarray(pwb, np.uint8).reshape(-1, 100)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2).copy()
        n = len(pwb)
        ok = np.empty(n, np.uint8)
        chi2 = np.empty(n, np.float32)
        patch = np.ascontiguousarray(pwb.reshape(n, 10, 10)[:, 1:9, 1:9]).reshape(n, 64)
        self._chk(self.lib.ygz_hip_align2d(self._ctx, cur_slot, level, _p(pwb, C.c_uint8), _p(patch, C.c_uint8), _p(uv, C.c_double),
                                           _p(ok, C.c_uint8), _p(chi2, C.c_float), n, n_iter), "align2d")
        return ok.astype(bool), uv, chi2

    def sparse_align(self, ref_slot, T_ref, cur_slot, T_cur, px, depth, has_mp, max_level=2, min_level=0, n_iter=30):
        Tr = (C.c_double * 7)(*T_ref)
        Tc = (C.c_double * 7)(*T_cur)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        depth = np.ascontiguousarray(depth, np.float64)
        has_mp = np.ascontiguousarray(has_mp, np.uint8)
        nm = C.c_int(0)
        iters = (C.c_int * MAX_LEVELS)()
        self._chk(self.lib.ygz_hip_sparse_align(self._ctx, ref_slot, Tr, cur_slot, Tc, _p(px, C.c_double), _p(depth, C.c_double),
                                                _p(has_mp, C.c_uint8), len(depth), max_level, min_level, n_iter, C.byref(nm), iters),
                  "sparse_align")
        return nm.value, np.array(list(Tc)), list(iters)[:self.levels]

    # ---- KLT
    def klt_params(self):
        p = KltParams()
        self.lib.ygz_hip_default_klt_params(C.byref(p))
        return p

    def klt_track(self, prev_slot, cur_slot, prev_pts, next_pts_init, params=None):
        prm = params or self.klt_params()
        pp = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        npts = np.ascontiguousarray(next_pts_init, np.float32).reshape(-1, 2).copy()
        st = np.empty(len(pp), np.uint8)
        err = np.empty(len(pp), np.float32)
        self._chk(self.lib.ygz_hip_klt_track(self._ctx, prev_slot, cur_slot, _p(pp, C.c_float), _p(npts, C.c_float), len(pp),
                                             C.byref(prm), _p(st, C.c_uint8), _p(err, C.c_float)), "klt_track")
        return npts, st, err

    def klt_track_filtered(self, prev_slot, cur_slot, prev_pts, next_pts_init, border=20, params=None):
        prm = params or self.klt_params()
        pp = np.ascontiguousarray(prev_pts, np.float32).reshape(-1, 2)
        npts = np.ascontiguousarray(next_pts_init, np.float32).reshape(-1, 2).copy()
        n = len(pp)
        st = np.empty(max(n, 1), np.uint8); err = np.empty(max(n, 1), np.float32); keep = np.zeros(max(n, 1), np.uint8); nk = C.c_int(0)
        self._chk(self.lib.ygz_hip_klt_track_filtered(self._ctx, prev_slot, cur_slot, _p(pp, C.c_float), _p(npts, C.c_float), n, C.byref(prm),
                                                      int(border), _p(st, C.c_uint8), _p(err, C.c_float), _p(keep, C.c_uint8), C.byref(nk)),
                  "klt_track_filtered")
        return npts, st[:n], err[:n], keep[:n].astype(bool), nk.value

    # ---- resident batched tracking
    def set_keypoint_depths(self, slot, depth, has_mp):
        depth = np.ascontiguousarray(depth, np.float64)
        has_mp = np.ascontiguousarray(has_mp, np.uint8)
        self._chk(self.lib.ygz_hip_set_keypoint_depths(self._ctx, slot, _p(depth, C.c_double), _p(has_mp, C.c_uint8), len(depth)),
                  "set_keypoint_depths")

    def track_begin(self, cur_slots, ref_slots, T_cur, T_ref, predict=True):
        c = np.ascontiguousarray(cur_slots, np.int32)
        r = np.ascontiguousarray(ref_slots, np.int32)
        Tc = np.ascontiguousarray(T_cur, np.float64).reshape(-1, 7)
        Tr = np.ascontiguousarray(T_ref, np.float64).reshape(-1, 7)
        self._chk(self.lib.ygz_hip_track_begin(self._ctx, _p(c, C.c_int32), _p(r, C.c_int32), _p(Tc, C.c_double), _p(Tr, C.c_double),
                                               len(c), int(predict)), "track_begin")

    def track_reload(self, predict=True):
        self._chk(self.lib.ygz_hip_track_reload(self._ctx, int(predict)), "track_reload")

    def track_klt_prepare(self):
        self._chk(self.lib.ygz_hip_track_klt_prepare(self._ctx), "track_klt_prepare")

    def track_klt(self, params=None):
        prm = params or self.klt_params()
        self._chk(self.lib.ygz_hip_track_klt(self._ctx, C.byref(prm)), "track_klt")

    def track_direct(self):
        self._chk(self.lib.ygz_hip_track_direct(self._ctx), "track_direct")

    def track_sparse_align(self, max_level=2, min_level=0, n_iter=30):
        self._chk(self.lib.ygz_hip_track_sparse_align(self._ctx, max_level, min_level, n_iter), "track_sparse_align")

    def track_adopt_pose(self):
        self._chk(self.lib.ygz_hip_track_adopt_pose(self._ctx), "track_adopt_pose")

    def track_pose_only(self):
        self._chk(self.lib.ygz_hip_track_pose_only(self._ctx), "track_pose_only")

    def track_get_pose_only(self, pair):
        pose = (C.c_double * 6)(); T = (C.c_double * 7)()
        inl, rnd, n = C.c_int(0), C.c_int(0), C.c_int(0)
        bad = np.zeros(self.cells, np.uint8); depth = np.zeros(self.cells, np.float64)
        self._chk(self.lib.ygz_hip_track_get_pose_only(self._ctx, pair, pose, T, C.byref(inl), C.byref(rnd), _p(bad, C.c_uint8),
                                                       _p(depth, C.c_double), self.cells, C.byref(n)), "track_get_pose_only")
        return dict(pose=np.array(list(pose)), T=np.array(list(T)), inliers=inl.value, rounds=rnd.value,
                    bad=bad[:n.value].astype(bool), depth=depth[:n.value].copy())

    def track_get_klt(self, pair):
        pts = np.empty((self.cells, 2), np.float32)
        st = np.empty(self.cells, np.uint8)
        err = np.empty(self.cells, np.float32)
        n = C.c_int(0)
        self._chk(self.lib.ygz_hip_track_get_klt(self._ctx, pair, _p(pts, C.c_float), _p(st, C.c_uint8), _p(err, C.c_float), self.cells,
                                                 C.byref(n)), "track_get_klt")
        return pts[:n.value].copy(), st[:n.value].copy(), err[:n.value].copy()

    def track_get_direct(self, pair):
        px = np.empty((self.cells, 2), np.float64)
        lvl = np.empty(self.cells, np.int32)
        ok = np.empty(self.cells, np.uint8)
        n = C.c_int(0)
        self._chk(self.lib.ygz_hip_track_get_direct(self._ctx, pair, _p(px, C.c_double), _p(lvl, C.c_int32), _p(ok, C.c_uint8), self.cells,
                                                    C.byref(n)), "track_get_direct")
        return ok[:n.value].astype(bool), px[:n.value].copy(), lvl[:n.value].copy()

    def track_get_pose(self, pair):
        T = (C.c_double * 7)()
        nm = C.c_int(0)
        iters = (C.c_int * MAX_LEVELS)()
        self._chk(self.lib.ygz_hip_track_get_pose(self._ctx, pair, T, C.byref(nm), iters), "track_get_pose")
        return nm.value, np.array(list(T)), list(iters)[:self.levels]

    def depth_filter_update(self, cur_slot, T_cur, ref_slot, T_refs, seeds, batch_counter, max_n_kfs=5, conv_thresh=100.0):
        """seeds: dict of kp [n,2] f32, octave, ref (index into ref_slot), frame_id (u64), a, b, mu, z_range, sigma2 (f32); a/b/mu/sigma2 come
        back updated (copies) together with state, z, matched_px, pos_world"""
        rs = np.ascontiguousarray(ref_slot, np.int32); Tr = np.ascontiguousarray(T_refs, np.float64).reshape(-1, 7)
        kp = np.ascontiguousarray(seeds["kp"], np.float32).reshape(-1, 2); n = len(kp)
        oc = np.ascontiguousarray(seeds["octave"], np.int32); sr = np.ascontiguousarray(seeds["ref"], np.int32)
        fid = np.ascontiguousarray(seeds["frame_id"], np.uint64)
        f = {k: np.ascontiguousarray(seeds[k], np.float32).copy() for k in ("a", "b", "mu", "z_range", "sigma2")}
        st = np.zeros(max(n, 1), np.int32); z = np.zeros(max(n, 1)); mp = np.zeros((max(n, 1), 2)); pw = np.zeros((max(n, 1), 3)); nu = C.c_int(0)
        fp = lambda k: _p(f[k], C.c_float)
        self._chk(self.lib.ygz_hip_depth_filter_update(self._ctx, cur_slot, (C.c_double * 7)(*T_cur), len(rs), _p(rs, C.c_int32), _p(Tr, C.c_double),
                                                       int(batch_counter), int(max_n_kfs), C.c_double(conv_thresh), n, _p(kp, C.c_float), _p(oc, C.c_int32),
                                                       _p(sr, C.c_int32), _p(fid, C.c_uint64), fp("a"), fp("b"), fp("mu"), fp("z_range"), fp("sigma2"),
                                                       _p(st, C.c_int32), _p(z, C.c_double), _p(mp, C.c_double), _p(pw, C.c_double), C.byref(nu)),
                  "depth_filter_update")
        return dict(a=f["a"], b=f["b"], mu=f["mu"], sigma2=f["sigma2"], state=st[:n], z=z[:n], matched_px=mp[:n], pos_world=pw[:n], updated=nu.value)

    def create_map_points(self, slot1, T1, slot2, T2, px1, level1, px2):
        p1 = np.ascontiguousarray(px1, np.float64).reshape(-1, 2); l1 = np.ascontiguousarray(level1, np.int32)
        p2 = np.ascontiguousarray(px2, np.float64).reshape(-1, 2).copy()
        n = len(l1)
        code = np.zeros(max(n, 1), np.int32); d1 = np.zeros(max(n, 1)); d2 = np.zeros(max(n, 1)); pw = np.zeros((max(n, 1), 3))
        sl = np.zeros(max(n, 1), np.int32); nc = C.c_int(0)
        self._chk(self.lib.ygz_hip_create_map_points(self._ctx, slot1, (C.c_double * 7)(*T1), slot2, (C.c_double * 7)(*T2), n, _p(p1, C.c_double),
                                                     _p(l1, C.c_int32), _p(p2, C.c_double), _p(code, C.c_int32), _p(d1, C.c_double),
                                                     _p(d2, C.c_double), _p(pw, C.c_double), _p(sl, C.c_int32), C.byref(nc)), "create_map_points")
        return dict(px2=p2, code=code[:n], depth1=d1[:n], depth2=d2[:n], pos_world=pw[:n], search_level=sl[:n], created=nc.value)

    def depth_from_triangulation(self, T_search_ref, f_ref, f_cur, determinant_th=1e-5):
        T = (C.c_double * 7)(*T_search_ref)
        fr = np.ascontiguousarray(f_ref, np.float64).reshape(-1, 3); fc = np.ascontiguousarray(f_cur, np.float64).reshape(-1, 3)
        n = len(fr)
        d1, d2, ok = np.full(max(n, 1), np.nan), np.full(max(n, 1), np.nan), np.zeros(max(n, 1), np.uint8)
        self.lib.ygz_hip_depth_from_triangulation.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                                              C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        self._chk(self.lib.ygz_hip_depth_from_triangulation(self._ctx, T, _p(fr, C.c_double), _p(fc, C.c_double), n, float(determinant_th),
                                                            _p(d1, C.c_double), _p(d2, C.c_double), _p(ok, C.c_uint8)), "depth_from_triangulation")
        return d1[:n], d2[:n], ok[:n]

    # ---- monocular initialisation (Initializer::TryInitialize)

    def _init_args(self, px1, px2):
        px1 = np.ascontiguousarray(px1, np.float64).reshape(-1, 2)
        px2 = np.ascontiguousarray(px2, np.float64).reshape(-1, 2)
        if len(px1) != len(px2):
            raise ValueError("px1 and px2 differ in length")
        return px1, px2, len(px1)

    def initialize(self, px1, px2, K4, **params):
        """the fused call (ygz_hip_initialize): dict of the result fields, pts3d [n][3], triangulated [n] (bool).  params: the fields of
        ygz_init_params (sigma, sigma2, max_iter, min_parallax, min_triangulated, good_point_ratio_h)"""
        px1, px2, n = self._init_args(px1, px2)
        K = (C.c_double * 4)(*[float(v) for v in K4])
        prm, res = _init_params(**params), InitResult()
        p3d, tri = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), np.uint8)
        self.lib.ygz_hip_initialize.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                                C.POINTER(InitParams), C.POINTER(InitResult), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        self._chk(self.lib.ygz_hip_initialize(self._ctx, _p(px1, C.c_double), _p(px2, C.c_double), n, K, C.byref(prm), C.byref(res),
                                              _p(p3d, C.c_double), _p(tri, C.c_uint8)), "initialize")
        d = res.to_dict()
        d["pts3d"], d["triangulated"] = p3d[:n], tri[:n].astype(bool)
        return d

    def init_hypotheses(self, px1, px2, **params):
        """every H / F hypothesis with its score, the winners' inlier masks and the model choice (ygz_hip_init_hypotheses)"""
        px1, px2, n = self._init_args(px1, px2)
        prm, res = _init_params(**params), InitResult()
        it = prm.max_iter
        H, F = np.zeros((max(it, 1), 3, 3)), np.zeros((max(it, 1), 3, 3))
        sh, sf = np.zeros(max(it, 1), np.float32), np.zeros(max(it, 1), np.float32)
        ih, jf = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        self.lib.ygz_hip_init_hypotheses.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(InitParams),
                                                     C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                     C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.POINTER(InitResult)]
        self._chk(self.lib.ygz_hip_init_hypotheses(self._ctx, _p(px1, C.c_double), _p(px2, C.c_double), n, C.byref(prm), _p(H, C.c_double),
                                                   _p(F, C.c_double), _p(sh, C.c_float), _p(sf, C.c_float), _p(ih, C.c_uint8), _p(jf, C.c_uint8),
                                                   C.byref(res)), "init_hypotheses")
        return dict(H21=H[:it], F21=F[:it], score_h=sh[:it], score_f=sf[:it], inliers_h=ih[:n].astype(bool), inliers_f=jf[:n].astype(bool),
                    result=res.to_dict())

    def init_reconstruct(self, px1, px2, K4, model, M, inliers, **params):
        """ReconstructH (model INIT_H, M = H21) / ReconstructF (INIT_F, M = F21) from a given model (ygz_hip_init_reconstruct)"""
        px1, px2, n = self._init_args(px1, px2)
        K = (C.c_double * 4)(*[float(v) for v in K4])
        Mm = (C.c_double * 9)(*[float(v) for v in np.asarray(M, np.float64).ravel()])
        inl = np.ascontiguousarray(inliers, np.uint8).reshape(-1)
        prm, res = _init_params(**params), InitResult()
        p3d, tri = np.zeros((max(n, 1), 3)), np.zeros(max(n, 1), np.uint8)
        self.lib.ygz_hip_init_reconstruct.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                                      C.POINTER(InitParams), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint8),
                                                      C.POINTER(InitResult), C.POINTER(C.c_double), C.POINTER(C.c_uint8)]
        self._chk(self.lib.ygz_hip_init_reconstruct(self._ctx, _p(px1, C.c_double), _p(px2, C.c_double), n, K, C.byref(prm), int(model), Mm,
                                                    _p(inl, C.c_uint8), C.byref(res), _p(p3d, C.c_double), _p(tri, C.c_uint8)), "init_reconstruct")
        d = res.to_dict()
        d["pts3d"], d["triangulated"] = p3d[:n], tri[:n].astype(bool)
        return d

    # ---- relocalisation pose (P3P RANSAC)

    def pnp_ransac(self, pw, px, offsets, K4, **params):
        """every problem p of offsets [P + 1] (correspondences offsets[p] .. offsets[p+1]-1 of pw [N][3], px [N][2]) in one call
        (ygz_hip_pnp_ransac): a list of result dicts and the inlier mask [N] (bool).  params: max_iter, chi2, min_inliers"""
        pw = np.ascontiguousarray(pw, np.float64).reshape(-1, 3)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        if len(pw) != len(px):
            raise ValueError("pw and px differ in length")
        P = len(off) - 1
        K = (C.c_double * 4)(*[float(v) for v in K4])
        prm = _pnp_params(**params)
        res = (PnpResult * max(P, 1))()
        inl = np.zeros(max(len(pw), 1), np.uint8)
        self.lib.ygz_hip_pnp_ransac.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                C.POINTER(C.c_double), C.POINTER(PnpParams), C.POINTER(PnpResult), C.POINTER(C.c_uint8)]
        self._chk(self.lib.ygz_hip_pnp_ransac(self._ctx, P, _p(off, C.c_int32), _p(pw, C.c_double), _p(px, C.c_double), K, C.byref(prm),
                                              res, _p(inl, C.c_uint8)), "pnp_ransac")
        return [res[i].to_dict() for i in range(P)], inl[:len(pw)].astype(bool)

    def pnp_hypotheses(self, pw, px, K4, **params):
        """every hypothesis of one problem (ygz_hip_pnp_hypotheses): solutions [max_iter][4][12] (R row-major, t), n_solutions [max_iter],
        counts [max_iter][4]"""
        pw = np.ascontiguousarray(pw, np.float64).reshape(-1, 3)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        if len(pw) != len(px):
            raise ValueError("pw and px differ in length")
        n = len(pw)
        K = (C.c_double * 4)(*[float(v) for v in K4])
        prm = _pnp_params(**params)
        it = max(prm.max_iter, 1)
        sol, ns, cnt = np.zeros((it, 4, 12)), np.zeros(it, np.int32), np.zeros((it, 4), np.int32)
        self.lib.ygz_hip_pnp_hypotheses.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                                    C.POINTER(PnpParams), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_pnp_hypotheses(self._ctx, _p(pw, C.c_double), _p(px, C.c_double), n, K, C.byref(prm), _p(sol, C.c_double),
                                                  _p(ns, C.c_int32), _p(cnt, C.c_int32)), "pnp_hypotheses")
        return dict(solutions=sol, n_solutions=ns, counts=cnt)

    # ---- loop detection (Sim3 RANSAC and refinement)

    @staticmethod
    def _sim3_arrays(X1, X2, px1, px2, levels):
        X1 = np.ascontiguousarray(X1, np.float64).reshape(-1, 3)
        X2 = np.ascontiguousarray(X2, np.float64).reshape(-1, 3)
        px1 = np.ascontiguousarray(px1, np.float64).reshape(-1, 2)
        px2 = np.ascontiguousarray(px2, np.float64).reshape(-1, 2)
        lv = np.ascontiguousarray(levels, np.int32).reshape(-1, 2)
        if not (len(X1) == len(X2) == len(px1) == len(px2) == len(lv)):
            raise ValueError("X1, X2, px1, px2 and levels differ in length")
        return X1, X2, px1, px2, lv

    def sim3_ransac(self, X1, X2, px1, px2, levels, offsets, K4, **params):
        """every problem p of offsets [P + 1] (pairs offsets[p] .. offsets[p+1]-1) in one call (ygz_hip_sim3_ransac): a list of result dicts
        and the mask [N] (uint8: bit 0 RANSAC inlier, bit 1 refined inlier).  params: the fields of ygz_sim3_params"""
        X1, X2, px1, px2, lv = self._sim3_arrays(X1, X2, px1, px2, levels)
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        P = len(off) - 1
        K = (C.c_double * 4)(*[float(v) for v in K4])
        prm = _sim3_params(**params)
        res = (Sim3Result * max(P, 1))()
        mask = np.zeros(max(len(X1), 1), np.uint8)
        dp = C.POINTER(C.c_double)
        self.lib.ygz_hip_sim3_ransac.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), dp, dp, dp, dp, C.POINTER(C.c_int32), dp,
                                                 C.POINTER(Sim3Params), C.POINTER(Sim3Result), C.POINTER(C.c_uint8)]
        self._chk(self.lib.ygz_hip_sim3_ransac(self._ctx, P, _p(off, C.c_int32), _p(X1, C.c_double), _p(X2, C.c_double), _p(px1, C.c_double),
                                               _p(px2, C.c_double), _p(lv, C.c_int32), K, C.byref(prm), res, _p(mask, C.c_uint8)), "sim3_ransac")
        return [res[i].to_dict() for i in range(P)], mask[:len(X1)]

    def sim3_hypotheses(self, X1, X2, px1, px2, levels, K4, **params):
        """every sample of one problem (ygz_hip_sim3_hypotheses): hyps [max_iter][16] (S12 then S21), valid [max_iter], counts [max_iter]"""
        X1, X2, px1, px2, lv = self._sim3_arrays(X1, X2, px1, px2, levels)
        K = (C.c_double * 4)(*[float(v) for v in K4])
        prm = _sim3_params(**params)
        it = max(prm.max_iter, 1)
        hyp, val, cnt = np.zeros((it, 16)), np.zeros(it, np.int32), np.zeros(it, np.int32)
        dp = C.POINTER(C.c_double)
        self.lib.ygz_hip_sim3_hypotheses.argtypes = [C.c_void_p, dp, dp, dp, dp, C.POINTER(C.c_int32), C.c_int, dp, C.POINTER(Sim3Params), dp,
                                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_sim3_hypotheses(self._ctx, _p(X1, C.c_double), _p(X2, C.c_double), _p(px1, C.c_double), _p(px2, C.c_double),
                                                   _p(lv, C.c_int32), len(X1), K, C.byref(prm), _p(hyp, C.c_double), _p(val, C.c_int32),
                                                   _p(cnt, C.c_int32)), "sim3_hypotheses")
        return dict(hyps=hyp, valid=val, counts=cnt)

    # ---- loop closing (descriptor search guided by projection)

    def search_by_projection(self, problems, K4, **params):
        """every problem (a dict, see proj_problems) in one call (ygz_hip_search_by_projection): match, dist, pred_level [N] concatenated over
        the problems and counts [P][2] (matches, overflowed points).  params: the fields of ygz_proj_params"""
        arr, keep = proj_problems(problems)
        P = len(problems)
        N = sum(int(arr[q].n_pt) for q in range(P))
        K = (C.c_double * 4)(*[float(v) for v in K4])
        prm = _proj_params(**params)
        match, dist, pred = (np.full(max(N, 1), -2, np.int32) for _ in range(3))
        counts = np.zeros((max(P, 1), 2), np.int32)
        ip = C.POINTER(C.c_int32)
        self.lib.ygz_hip_search_by_projection.argtypes = [C.c_void_p, C.c_int, C.POINTER(ProjProblem), C.POINTER(C.c_double), C.POINTER(ProjParams),
                                                          ip, ip, ip, ip]
        self._chk(self.lib.ygz_hip_search_by_projection(self._ctx, P, arr, K, C.byref(prm), _p(match, C.c_int32), _p(dist, C.c_int32),
                                                        _p(pred, C.c_int32), _p(counts, C.c_int32)), "search_by_projection")
        del keep
        return dict(match=match[:N], dist=dist[:N], pred_level=pred[:N], counts=counts[:P])

    def projection_candidates(self, problem, K4, **params):
        """the candidate lists of one problem before any claim (ygz_hip_projection_candidates): cand_idx, cand_dist [n_pt][8], n_cand [n_pt],
        pred_level [n_pt]"""
        arr, keep = proj_problems([problem])
        n = int(arr[0].n_pt)
        K = (C.c_double * 4)(*[float(v) for v in K4])
        prm = _proj_params(**params)
        ci, cd = np.full((max(n, 1), PROJ_TOPK), -2, np.int32), np.full((max(n, 1), PROJ_TOPK), -2, np.int32)
        nc, pred = np.full(max(n, 1), -2, np.int32), np.full(max(n, 1), -2, np.int32)
        ip = C.POINTER(C.c_int32)
        self.lib.ygz_hip_projection_candidates.argtypes = [C.c_void_p, C.POINTER(ProjProblem), C.POINTER(C.c_double), C.POINTER(ProjParams),
                                                           ip, ip, ip, ip]
        self._chk(self.lib.ygz_hip_projection_candidates(self._ctx, arr, K, C.byref(prm), _p(ci, C.c_int32), _p(cd, C.c_int32), _p(nc, C.c_int32),
                                                         _p(pred, C.c_int32)), "projection_candidates")
        del keep
        return dict(cand_idx=ci[:n], cand_dist=cd[:n], n_cand=nc[:n], pred_level=pred[:n])

    # ---- loop correction (Sim3 pose-graph optimisation)

    def pose_graph_optimize(self, S, fixed, edges, M, **params):
        """the whole optimisation in one call (ygz_hip_pose_graph_optimize): dict(S [N][8], and the fields of ygz_pgo_result).  params: the
        fields of ygz_pgo_params"""
        S, fixed, edges, M = pgo_arrays(S, fixed, edges, M)
        prm, res, out = _pgo_params(**params), PgoResult(), np.zeros_like(S)
        pgo_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_pose_graph_optimize(self._ctx, len(S), _p(S, C.c_double), _p(fixed, C.c_uint8), len(edges), _p(edges, C.c_int32),
                                                       _p(M, C.c_double), C.byref(prm), _p(out, C.c_double), C.byref(res)), "pose_graph_optimize")
        d = res.to_dict()
        d["S"] = out
        return d

    def pgo_linearize(self, S, fixed, edges, M, **params):
        """the linearisation at S (ygz_hip_pgo_linearize): dict(ok, res [E][7], Ji, Jj [E][7][7], cost); ok is False when the residual is
        undefined at S"""
        S, fixed, edges, M = pgo_arrays(S, fixed, edges, M)
        E = len(edges)
        prm = _pgo_params(**params)
        res, Ji, Jj, cost = np.zeros((E, 7)), np.zeros((E, 7, 7)), np.zeros((E, 7, 7)), np.zeros(1)
        pgo_argtypes(self.lib)
        rc = self.lib.ygz_hip_pgo_linearize(self._ctx, len(S), _p(S, C.c_double), _p(fixed, C.c_uint8), E, _p(edges, C.c_int32), _p(M, C.c_double),
                                            C.byref(prm), _p(res, C.c_double), _p(Ji, C.c_double), _p(Jj, C.c_double), _p(cost, C.c_double))
        if rc != E_STATE:
            self._chk(rc, "pgo_linearize")
        return dict(ok=rc == OK, res=res, Ji=Ji, Jj=Jj, cost=float(cost[0]))

    # ---- global bundle adjustment after a loop closing

    def global_ba(self, poses, fixed, points, edge_pose, edge_point, obs, K4, huber_delta=GBA_HUBER, **params):
        """the whole optimisation in one call (ygz_hip_global_ba): dict(poses [N][7], points [L][3], and the fields of ygz_gba_result).
        params: the fields of ygz_gba_params; cg_batch is the number of CG iterations queued per read-back (no output depends on it)"""
        poses, fixed, points, ep, el, obs = gba_arrays(poses, fixed, points, edge_pose, edge_point, obs)
        K = np.ascontiguousarray(K4, np.float64).reshape(4)
        prm, res, po, xo = _gba_params(**params), GbaResult(), np.zeros_like(poses), np.zeros_like(points)
        gba_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_global_ba(self._ctx, len(poses), _p(poses, C.c_double), _p(fixed, C.c_uint8), len(points), _p(points, C.c_double),
                                             len(ep), _p(ep, C.c_int32), _p(el, C.c_int32), _p(obs, C.c_double), _p(K, C.c_double), float(huber_delta),
                                             C.byref(prm), _p(po, C.c_double), _p(xo, C.c_double), C.byref(res)), "global_ba")
        d = res.to_dict()
        d["poses"], d["points"] = po, xo
        return d

    def gba_linearize(self, poses, fixed, points, edge_pose, edge_point, obs, K4, huber_delta=GBA_HUBER, **params):
        """the linearisation at the input (ygz_hip_gba_linearize): dict(ok, res [E][2], w [E], Jp [E][2][6], Jl [E][2][3], Hpp [N][21], bp
        [N][6], Hll [L][6], bl [L][3], cost); ok is False when a residual is undefined"""
        poses, fixed, points, ep, el, obs = gba_arrays(poses, fixed, points, edge_pose, edge_point, obs)
        K = np.ascontiguousarray(K4, np.float64).reshape(4)
        N, L, E = len(poses), len(points), len(ep)
        prm = _gba_params(**params)
        o = dict(res=np.zeros((E, 2)), w=np.zeros(E), Jp=np.zeros((E, 2, 6)), Jl=np.zeros((E, 2, 3)), Hpp=np.zeros((N, 21)), bp=np.zeros((N, 6)),
                 Hll=np.zeros((L, 6)), bl=np.zeros((L, 3)))
        cost = np.zeros(1)
        gba_argtypes(self.lib)
        rc = self.lib.ygz_hip_gba_linearize(self._ctx, N, _p(poses, C.c_double), _p(fixed, C.c_uint8), L, _p(points, C.c_double), E, _p(ep, C.c_int32),
                                            _p(el, C.c_int32), _p(obs, C.c_double), _p(K, C.c_double), float(huber_delta), C.byref(prm),
                                            *[_p(o[k], C.c_double) for k in ("res", "w", "Jp", "Jl", "Hpp", "bp", "Hll", "bl")], _p(cost, C.c_double))
        if rc != E_STATE:
            self._chk(rc, "gba_linearize")
        o.update(ok=rc == OK, cost=float(cost[0]))
        return o

    # ---- stereo bundle adjustment

    def default_sba_params(self):
        """ygz_hip_default_sba_params as a dict"""
        p = default_sba_params()
        return dict((k, list(getattr(p, k)) if k == "iterations" else getattr(p, k)) for k, _ in p._fields_)

    def stereo_ba(self, poses, fixed, points, edge_pose, edge_point, obs, kind, level, K4, want_flags=True, **params):
        """mono and stereo edges, rounds of LM with the edges classified in between (ygz_hip_stereo_ba): dict(poses [N][7], points [L][3],
        outlier [E], chi2 [E] (None without want_flags: NULL is passed), rounds_run and the per-round arrays of ygz_sba_result).  params: the
        fields of ygz_sba_params; iterations is a list of up to four"""
        poses, fixed, points, ep, el, obs, kind, level = sba_arrays(poses, fixed, points, edge_pose, edge_point, obs, kind, level)
        K = np.ascontiguousarray(K4, np.float64).reshape(4)
        prm, res, po, xo = _sba_params(**params), SbaResult(), np.zeros_like(poses), np.zeros_like(points)
        out, chi2 = (np.zeros(len(ep), np.uint8), np.zeros(len(ep))) if want_flags else (None, None)
        sba_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_stereo_ba(self._ctx, len(poses), _p(poses, C.c_double), _p(fixed, C.c_uint8), len(points), _p(points, C.c_double),
                                             len(ep), _p(ep, C.c_int32), _p(el, C.c_int32), _p(obs, C.c_double), _p(kind, C.c_uint8),
                                             _p(level, C.c_int32), _p(K, C.c_double), C.byref(prm), _p(po, C.c_double), _p(xo, C.c_double),
                                             _p(out, C.c_uint8) if want_flags else None, _p(chi2, C.c_double) if want_flags else None,
                                             C.byref(res)), "stereo_ba")
        d = res.to_dict()
        d.update(poses=po, points=xo, outlier=out, chi2=chi2)
        return d

    def sba_linearize(self, poses, fixed, points, edge_pose, edge_point, obs, kind, level, K4, **params):
        """the linearisation at the input (ygz_hip_sba_linearize): dict(ok, res [E][3], w [E], Jp [E][3][6], Jl [E][3][3], Hpp [N][21], bp
        [N][6], Hll [L][6], bl [L][3], cost); ok is False when a present edge is undefined"""
        poses, fixed, points, ep, el, obs, kind, level = sba_arrays(poses, fixed, points, edge_pose, edge_point, obs, kind, level)
        K = np.ascontiguousarray(K4, np.float64).reshape(4)
        N, L, E = len(poses), len(points), len(ep)
        prm = _sba_params(**params)
        o = dict(res=np.zeros((E, 3)), w=np.zeros(E), Jp=np.zeros((E, 3, 6)), Jl=np.zeros((E, 3, 3)), Hpp=np.zeros((N, 21)), bp=np.zeros((N, 6)),
                 Hll=np.zeros((L, 6)), bl=np.zeros((L, 3)))
        cost = np.zeros(1)
        sba_argtypes(self.lib)
        rc = self.lib.ygz_hip_sba_linearize(self._ctx, N, _p(poses, C.c_double), _p(fixed, C.c_uint8), L, _p(points, C.c_double), E, _p(ep, C.c_int32),
                                            _p(el, C.c_int32), _p(obs, C.c_double), _p(kind, C.c_uint8), _p(level, C.c_int32), _p(K, C.c_double),
                                            C.byref(prm), *[_p(o[k], C.c_double) for k in ("res", "w", "Jp", "Jl", "Hpp", "bp", "Hll", "bl")],
                                            _p(cost, C.c_double))
        if rc != E_STATE:
            self._chk(rc, "sba_linearize")
        o.update(ok=rc == OK, cost=float(cost[0]))
        return o

    # ---- map upkeep after a loop correction

    def distinctive_descriptors(self, offsets, desc):
        """ORB-SLAM2's ComputeDistinctiveDescriptors for a batch of points (ygz_hip_distinctive_descriptors): offsets [P + 1], desc
        [n_obs][32]; dict(best [P], median [P], desc [P][32])"""
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        P = len(off) - 1
        if P < 1 or int(off[-1]) != len(d):
            raise ValueError("offsets do not describe desc")
        d = d if len(d) else np.zeros((1, 32), np.uint8)
        best, med, out = np.full(P, -2, np.int32), np.full(P, -2, np.int32), np.full((P, 32), 0xAA, np.uint8)
        map_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_distinctive_descriptors(self._ctx, P, _p(off, C.c_int32), _p(d, C.c_uint8), _p(best, C.c_int32),
                                                           _p(med, C.c_int32), _p(out, C.c_uint8)), "distinctive_descriptors")
        return dict(best=best, median=med, desc=out)

    def covisibility(self, offsets, kf, n_keyframes, rows):
        """shared-point counts (ygz_hip_covisibility): offsets [P + 1], kf [n_obs] ascending within a point, rows [R] distinct keyframe
        indices; weights [R][n_keyframes]"""
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        k = np.ascontiguousarray(kf, np.int32).reshape(-1)
        r = np.ascontiguousarray(rows, np.int32).reshape(-1)
        P = len(off) - 1
        if P < 1 or int(off[-1]) != len(k):
            raise ValueError("offsets do not describe kf")
        k = k if len(k) else np.zeros(1, np.int32)
        w = np.full((max(len(r), 1), max(int(n_keyframes), 1)), -2, np.int32)
        map_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_covisibility(self._ctx, P, _p(off, C.c_int32), _p(k, C.c_int32), int(n_keyframes), len(r), _p(r, C.c_int32),
                                                _p(w, C.c_int32)), "covisibility")
        return w

    # ---- keyframe culling

    def keyframe_redundancy(self, offsets, kf, level, n_keyframes, **params):
        """the culling counts of every keyframe (ygz_hip_keyframe_redundancy): offsets [P + 1], kf [n_obs] ascending within a point, level
        [n_obs]; params: the fields of ygz_cull_params; dict(tracked [K], redundant [K])"""
        off, k, l = cull_arrays(offsets, kf, level)
        K = int(n_keyframes)
        prm = _cull_params(**params)
        t, r = np.full(max(K, 1), -2, np.int32), np.full(max(K, 1), -2, np.int32)
        cull_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_keyframe_redundancy(self._ctx, len(off) - 1, _p(off, C.c_int32), _p(k, C.c_int32), _p(l, C.c_int32), K,
                                                       C.byref(prm), _p(t, C.c_int32), _p(r, C.c_int32)), "keyframe_redundancy")
        return dict(tracked=t, redundant=r)

    def cull_keyframes(self, offsets, kf, level, n_keyframes, cand, **params):
        """ORB-SLAM2's culling walk over the candidates in the order given (ygz_hip_cull_keyframes); dict(culled, tracked, redundant
        [n_cand], point_dead [P] uint8)"""
        off, k, l = cull_arrays(offsets, kf, level)
        c = np.ascontiguousarray(cand, np.int32).reshape(-1)
        n, P = len(c), len(off) - 1
        prm = _cull_params(**params)
        o = dict(culled=np.full(max(n, 1), -2, np.int32), tracked=np.full(max(n, 1), -2, np.int32), redundant=np.full(max(n, 1), -2, np.int32),
                 point_dead=np.full(P, 0xAA, np.uint8))
        c = c if n else np.zeros(1, np.int32)
        cull_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_cull_keyframes(self._ctx, P, _p(off, C.c_int32), _p(k, C.c_int32), _p(l, C.c_int32), int(n_keyframes), n,
                                                  _p(c, C.c_int32), C.byref(prm), _p(o["culled"], C.c_int32), _p(o["tracked"], C.c_int32),
                                                  _p(o["redundant"], C.c_int32), _p(o["point_dead"], C.c_uint8)), "cull_keyframes")
        return o

    # ---- local-map selection

    def local_map_select(self, kf_bad, cov, offsets, kf, feat, frame_offsets, frame_points, pt_bad=None, outputs=None, **params):
        """the local keyframes and local points of many frames on one map (ygz_hip_local_map_select): kf_bad [K], cov [K][C] (-1: none),
        offsets [P + 1], kf and feat [n_obs], frame_offsets [F + 1], frame_points [E] (-1: no point), pt_bad [P] or None; params: the fields
        of ygz_lms_params; outputs: the names of LMS_OUTPUTS to bring back (None: all; n_local and local_kf always).  dict of int32 arrays:
        votes, local_kf [F][K], ref, n_voters, n_local, n_pt, n_cut [F], local_pt [F][max_points], fr_prior [E]"""
        one = lambda a: a if len(a) else np.zeros(1, np.int32)
        bad = np.ascontiguousarray(kf_bad, np.uint8).reshape(-1)
        K = len(bad)
        cv = np.ascontiguousarray(cov, np.int32).reshape(K, -1)
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        k, ft = np.ascontiguousarray(kf, np.int32).reshape(-1), np.ascontiguousarray(feat, np.int32).reshape(-1)
        fo, fp = np.ascontiguousarray(frame_offsets, np.int32).reshape(-1), np.ascontiguousarray(frame_points, np.int32).reshape(-1)
        if len(off) < 2 or len(fo) < 2 or int(off[-1]) != len(k) or len(k) != len(ft) or int(fo[-1]) != len(fp):
            raise ValueError("the offsets do not describe their arrays")
        pb = None if pt_bad is None else np.ascontiguousarray(pt_bad, np.uint8).reshape(-1)
        if pb is not None and len(pb) != len(off) - 1:
            raise ValueError("pt_bad has one entry per point")
        lms_argtypes(self.lib)
        prm = LmsParams()
        self.lib.ygz_hip_default_lms_params(C.byref(prm))
        for name, v in params.items():
            getattr(prm, name)
            setattr(prm, name, v)
        F, E, mp = len(fo) - 1, len(fp), max(int(prm.max_points), 1)
        shape = dict(votes=(F, K), ref=(F,), n_voters=(F,), n_local=(F,), local_kf=(F, K), n_pt=(F,), n_cut=(F,), local_pt=(F, mp), fr_prior=(max(E, 1),))
        want = set(LMS_OUTPUTS if outputs is None else outputs) | {"n_local", "local_kf"}
        o = {name: np.full(shape[name], -7, np.int32) for name in LMS_OUTPUTS if name in want}
        cv1, k1, ft1, fp1 = one(cv.reshape(-1)), one(k), one(ft), one(fp)
        self._chk(self.lib.ygz_hip_local_map_select(self._ctx, K, _p(bad, C.c_uint8), cv.shape[1], _p(cv1, C.c_int32), len(off) - 1,
                                                    _p(off, C.c_int32), _p(k1, C.c_int32), _p(ft1, C.c_int32),
                                                    None if pb is None else _p(pb, C.c_uint8), F, _p(fo, C.c_int32), _p(fp1, C.c_int32),
                                                    C.byref(prm), *[_p(o[name], C.c_int32) if name in o else None for name in LMS_OUTPUTS]),
                  "local_map_select")
        if "fr_prior" in o:
            o["fr_prior"] = o["fr_prior"][:E]
        return o

    # ---- map-point attributes and local-map tracking on an indexed map

    def map_point_attributes(self, kf_center, pw, offsets, obs_kf, obs_level):
        """dmax [P], normal [P, 3] and state [P] of every point of a map (ygz_hip_map_point_attributes): kf_center [K, 3], pw [P, 3], offsets
        [P + 1], obs_kf and obs_level [n_obs] in the caller's row order.  state 0: no row, 2: a distance of 0 or an output that is not
        finite (zeros are written), 1: usable"""
        c, x = np.ascontiguousarray(kf_center, np.float64).reshape(-1, 3), np.ascontiguousarray(pw, np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        k, lv = np.ascontiguousarray(obs_kf, np.int32).reshape(-1), np.ascontiguousarray(obs_level, np.int32).reshape(-1)
        if len(off) != len(x) + 1 or len(k) != len(lv) or (len(off) and int(off[-1]) != len(k)):
            raise ValueError("the offsets do not describe their arrays")
        P = len(x)
        o = dict(dmax=np.full(max(P, 1), -7.0), normal=np.full((max(P, 1), 3), -7.0), state=np.full(max(P, 1), -7, np.int32))
        one = lambda a, t: a if len(a) else np.zeros(3, t)
        mpa_argtypes(self.lib)
        self._chk(self.lib.ygz_hip_map_point_attributes(self._ctx, len(c), _p(one(c, np.float64), C.c_double), P, _p(one(x, np.float64), C.c_double),
                                                        _p(off, C.c_int32), _p(one(k, np.int32), C.c_int32), _p(one(lv, np.int32), C.c_int32),
                                                        _p(o["dmax"], C.c_double), _p(o["normal"], C.c_double), _p(o["state"], C.c_int32)),
                  "map_point_attributes")
        return {name: v[:P] for name, v in o.items()}

    def stereo_local_map_indexed(self, points, list_pt, list_len, slots, list_index, T, prior=None, params=None, outputs=True, **fields):
        """stereo_local_map_slots with the sets given as index lists into one map (ygz_hip_stereo_local_map_indexed).  points: dict of pw
        [P, 3], pt_desc [P, 32], pt_dmax [P], pt_normal [P, 3] (an empty dict: a map of 0 points); list_pt [n_lists, stride] and list_len
        [n_lists] as local_map_select writes local_pt and n_pt (the entries past list_len are not read); frame f has the keypoints of
        slots[f] and the points of list list_index[f].  The result is that of stereo_local_map_slots on the gathered sets."""
        p = params if params is not None else self.default_slm_params(**fields)
        slm_indexed_argtypes(self.lib)
        P = len(np.asarray(points["pt_desc"]).reshape(-1)) // 32 if points.get("pt_desc") is not None else 0

        def arr(name, t, n):
            a = points.get(name)
            if a is None:
                return None
            a = np.ascontiguousarray(a, t).reshape(-1)
            if len(a) != n:
                raise ValueError("%s has the wrong length" % name)
            return a
        m_pw, m_desc = arr("pw", np.float64, 3 * P), arr("pt_desc", np.uint8, 32 * P)
        m_dmax, m_nrm = arr("pt_dmax", np.float64, P), arr("pt_normal", np.float64, 3 * P)
        ll = np.ascontiguousarray(list_len, np.int32).reshape(-1)
        lp = np.ascontiguousarray(list_pt, np.int32).reshape(max(len(ll), 1), -1)
        stride = lp.shape[1]
        sl, li = np.ascontiguousarray(slots, np.int32).reshape(-1), np.ascontiguousarray(list_index, np.int32).reshape(-1)
        if len(sl) != len(li):
            raise ValueError("slots and list_index differ in length")
        n, c, R = len(sl), self.cells, POPT_MAX_ROUNDS
        T0 = np.ascontiguousarray(T, np.float64).reshape(n, 7)
        pr = None if prior is None else np.ascontiguousarray(prior, np.int32).reshape(n, c)
        off = [0]
        for f in range(n):
            off.append(off[-1] + (max(int(ll[int(li[f])]), 0) if 0 <= li[f] < len(ll) else 0))
        N, m = off[-1], max(n, 1)
        o = dict(T_out=np.zeros((m, 7)), status=np.full(m, -7, np.int32))
        names = ("counts", "kp_point", "outlier", "chi2", "inliers", "rounds_run", "round_status", "lm_iterations", "cost_initial", "cost_final",
                 "lambda") + SLM_INT_OUTPUTS + ("proj",)
        if outputs:
            o.update(counts=np.full((m, 8), -7, np.int32), kp_point=np.full((m, c), -7, np.int32), outlier=np.full((m, c), 7, np.uint8),
                     chi2=np.zeros((m, c)), inliers=np.full(m, -7, np.int32), rounds_run=np.full(m, -7, np.int32),
                     round_status=np.full((m, R), -7, np.int32), lm_iterations=np.full((m, R), -7, np.int32), cost_initial=np.zeros((m, R)),
                     cost_final=np.zeros((m, R)), proj=np.zeros((max(N, 1), 3)))
            o["lambda"] = np.zeros((m, R))
            for k in SLM_INT_OUTPUTS:
                o[k] = np.full(max(N, 1), -7, np.int32)
        types = {np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}
        f_ = lambda k: _p(o[k], types[o[k].dtype]) if k in o else None
        q_ = lambda a, t: None if a is None else _p(a, t)
        self._chk(self.lib.ygz_hip_stereo_local_map_indexed(
            self._ctx, P, q_(m_pw, C.c_double), q_(m_desc, C.c_uint8), q_(m_dmax, C.c_double), q_(m_nrm, C.c_double), len(ll), stride,
            _p(lp, C.c_int32), _p(ll, C.c_int32), n, _p(sl, C.c_int32), _p(li, C.c_int32), _p(T0, C.c_double), q_(pr, C.c_int32),
            C.byref(p), f_("T_out"), f_("status"), *[f_(k) for k in names]), "stereo_local_map_indexed")
        per_point = SLM_INT_OUTPUTS + ("proj",)
        out = {k: (v[:N] if k in per_point else v[:n]) for k, v in o.items()}
        out["offsets"] = np.array(off, np.int64)
        return out

    # ---- the resident map

    def map_create(self):
        """a resident map of this context (ygz_hip_map_create): see ResidentMap"""
        return ResidentMap(self)

    def stereo_local_map_resident(self, rmap, slots, T, frame_offsets, frame_points, lms=None, params=None, outputs=True, fill=None, **fields):
        """local-map selection and tracking of resident frames on a resident map in one device call (ygz_hip_stereo_local_map_resident).
        frame_offsets [F + 1] and frame_points [E] as local_map_select takes them; lms: dict of ygz_lms_params fields; params / fields: the
        ygz_slm_params.  The per-point outputs are [F, max_points] (proj [F, max_points, 3]); row f holds n_pt[f] entries, the rest keep the
        fill value.  fill: dict name -> value the outputs are pre-filled with (tests)."""
        p = params if params is not None else self.default_slm_params(**fields)
        lms_argtypes(self.lib)
        rmap_argtypes(self.lib)
        q = LmsParams()
        self.lib.ygz_hip_default_lms_params(C.byref(q))
        for name, v in (lms or {}).items():
            getattr(q, name)
            setattr(q, name, v)
        sl = np.ascontiguousarray(slots, np.int32).reshape(-1)
        fo, fp = np.ascontiguousarray(frame_offsets, np.int32).reshape(-1), np.ascontiguousarray(frame_points, np.int32).reshape(-1)
        n, c, R, K, mp = len(sl), self.cells, POPT_MAX_ROUNDS, max(rmap.info()["n_keyframes"], 1), max(int(q.max_points), 1)
        if len(fo) != n + 1:
            raise ValueError("frame_offsets has one entry per frame and one more")
        T0 = np.ascontiguousarray(T, np.float64).reshape(n, 7)
        m = max(n, 1)
        o = dict(T_out=np.zeros((m, 7)), status=np.full(m, -7, np.int32))
        sel = dict(votes=(m, K), ref=(m,), n_voters=(m,), n_local=(m,), local_kf=(m, K), n_cut=(m,), n_pt=(m,), local_pt=(m, mp), n_removed=(m,),
                   prior=(m, c))
        names = ("counts", "kp_point", "outlier", "chi2", "inliers", "rounds_run", "round_status", "lm_iterations", "cost_initial", "cost_final",
                 "lambda") + SLM_INT_OUTPUTS + ("proj",)
        if outputs:
            for k, shp in sel.items():
                o[k] = np.full(shp, -7, np.int32)
            o.update(counts=np.full((m, 8), -7, np.int32), kp_point=np.full((m, c), -7, np.int32), outlier=np.full((m, c), 7, np.uint8),
                     chi2=np.zeros((m, c)), inliers=np.full(m, -7, np.int32), rounds_run=np.full(m, -7, np.int32),
                     round_status=np.full((m, R), -7, np.int32), lm_iterations=np.full((m, R), -7, np.int32), cost_initial=np.zeros((m, R)),
                     cost_final=np.zeros((m, R)), proj=np.full((m, mp, 3), -7.0))
            o["lambda"] = np.zeros((m, R))
            for k in SLM_INT_OUTPUTS:
                o[k] = np.full((m, mp), -7, np.int32)
        for k, v in (fill or {}).items():
            o[k][...] = v
        types = {np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}
        f_ = lambda k: _p(o[k], types[o[k].dtype]) if k in o else None
        fp1 = fp if len(fp) else np.zeros(1, np.int32)
        rc = self.lib.ygz_hip_stereo_local_map_resident(
            self._ctx, rmap._map, n, _p(sl, C.c_int32), _p(T0, C.c_double), _p(fo, C.c_int32), _p(fp1, C.c_int32), C.byref(q), C.byref(p),
            *[f_(k) for k in RMAP_SELECT_OUTPUTS], f_("T_out"), f_("status"), *[f_(k) for k in names])
        self.last_outputs = o                                     # what a refused call left in the arrays (tests)
        self._chk(rc, "stereo_local_map_resident")
        return {k: v[:n] for k, v in o.items()}

    # ---- BoW
    def vocab_load(self, blob):
        buf = np.frombuffer(blob, np.uint8).copy()
        self._chk(self.lib.ygz_hip_vocab_load(self._ctx, _p(buf, C.c_uint8), C.c_size_t(len(buf))), "vocab_load")
        k, L, nn, nw = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.ygz_hip_vocab_info(self._ctx, C.byref(k), C.byref(L), C.byref(nn), C.byref(nw)), "vocab_info")
        return k.value, L.value, nn.value, nw.value

    def compute_bow(self, slot_begin, n_slots, levelsup=4):
        self._chk(self.lib.ygz_hip_compute_bow(self._ctx, slot_begin, n_slots, levelsup), "compute_bow")

    def get_bow(self, slot):
        word, weight, node = np.empty(self.cells, np.int32), np.empty(self.cells), np.empty(self.cells, np.int32)
        n = C.c_int(0)
        self._chk(self.lib.ygz_hip_get_bow(self._ctx, slot, _p(word, C.c_int32), _p(weight, C.c_double), _p(node, C.c_int32), self.cells,
                                           C.byref(n)), "get_bow")
        return word[:n.value].copy(), weight[:n.value].copy(), node[:n.value].copy()

    def bow_transform(self, desc, levelsup=4):
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        word, weight, node = np.empty(max(n, 1), np.int32), np.empty(max(n, 1)), np.empty(max(n, 1), np.int32)
        self._chk(self.lib.ygz_hip_bow_transform(self._ctx, _p(desc, C.c_uint8), n, levelsup, _p(word, C.c_int32), _p(weight, C.c_double),
                                                 _p(node, C.c_int32)), "bow_transform")
        return word[:n], weight[:n], node[:n]

    def search_by_bow_slots(self, slot1, slot2, mode=0, E12=None, th_low=65, knn_ratio=0.7, epipolar_dsqr=1e-4):
        s1 = np.ascontiguousarray(slot1, np.int32); s2 = np.ascontiguousarray(slot2, np.int32)
        n = len(s1)
        m = np.empty((n, self.cells), np.int32); cnt = np.empty(n, np.int32)
        E = None if E12 is None else np.ascontiguousarray(E12, np.float64).reshape(n, 9)
        self.lib.ygz_hip_search_by_bow_slots.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                         C.c_int, C.c_float, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_search_by_bow_slots(self._ctx, mode, n, _p(s1, C.c_int32), _p(s2, C.c_int32), None if E is None else _p(E, C.c_double),
                                                       int(th_low), float(knn_ratio), float(epipolar_dsqr), _p(m, C.c_int32), _p(cnt, C.c_int32)),
                  "search_by_bow_slots")
        return m, cnt

    def search_by_bow(self, desc1, node1, desc2, node2, mode=0, px1=None, px2=None, E12=None, th_low=65, knn_ratio=0.7, epipolar_dsqr=1e-4):
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        n1a = np.ascontiguousarray(node1, np.int32); n2a = np.ascontiguousarray(node2, np.int32)
        p1 = None if px1 is None else np.ascontiguousarray(px1, np.float64); p2 = None if px2 is None else np.ascontiguousarray(px2, np.float64)
        E = None if E12 is None else np.ascontiguousarray(E12, np.float64).reshape(9)
        m = np.empty(max(len(d1), 1), np.int32); cnt = C.c_int(0)
        f64 = lambda a: None if a is None else _p(a, C.c_double)
        self.lib.ygz_hip_search_by_bow.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int,
                                                   C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double),
                                                   C.c_int, C.c_float, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int)]
        self._chk(self.lib.ygz_hip_search_by_bow(self._ctx, mode, _p(d1, C.c_uint8), _p(n1a, C.c_int32), f64(p1), len(d1), _p(d2, C.c_uint8),
                                                 _p(n2a, C.c_int32), f64(p2), len(d2), f64(E), int(th_low), float(knn_ratio), float(epipolar_dsqr),
                                                 _p(m, C.c_int32), C.byref(cnt)), "search_by_bow")
        return m[:len(d1)], cnt.value

    def bow_orientation(self, angle1, angle2, match12):
        """Matcher::Options::checkOrientation on a SearchByBoW result: (count, hist [30], maxima [3])"""
        a1 = np.ascontiguousarray(angle1, np.float64); a2 = np.ascontiguousarray(angle2, np.float64); m = np.ascontiguousarray(match12, np.int32)
        kept = C.c_int(0); hist = np.zeros(30, np.int32); ind = np.zeros(3, np.int32)
        self.lib.ygz_hip_bow_orientation.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int32),
                                                     C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_bow_orientation(self._ctx, _p(a1, C.c_double), len(a1), _p(a2, C.c_double), len(a2), _p(m, C.c_int32), C.byref(kept),
                                                   _p(hist, C.c_int32), _p(ind, C.c_int32)), "bow_orientation")
        return kept.value, hist, ind

    def bow_orientation_slots(self, slot1, slot2, match12):
        s1 = np.ascontiguousarray(slot1, np.int32); s2 = np.ascontiguousarray(slot2, np.int32); m = np.ascontiguousarray(match12, np.int32)
        n = len(s1)
        assert m.shape == (n, self.cells)
        kept = np.zeros(n, np.int32); hist = np.zeros((n, 30), np.int32); ind = np.zeros((n, 3), np.int32)
        self.lib.ygz_hip_bow_orientation_slots.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        self._chk(self.lib.ygz_hip_bow_orientation_slots(self._ctx, n, _p(s1, C.c_int32), _p(s2, C.c_int32), _p(m, C.c_int32), _p(kept, C.c_int32),
                                                         _p(hist, C.c_int32), _p(ind, C.c_int32)), "bow_orientation_slots")
        return kept, hist, ind

    # ---- BA
    def _ba_problem(self, poses, fixed, points, edge_pose, edge_point, obs, huber_delta, formulation, cam=None,
                    point_fixed=None, edge_huber=None, edge_enable=None):
        if fixed is None:
            fixed = np.zeros(len(poses), np.uint8)
        self._keep = [np.ascontiguousarray(poses, np.float64).reshape(-1, 6), np.ascontiguousarray(fixed, np.uint8),
                      np.ascontiguousarray(points, np.float64).reshape(-1, 3), np.ascontiguousarray(edge_pose, np.int32),
                      np.ascontiguousarray(edge_point, np.int32), np.ascontiguousarray(obs, np.float64),
                      None if point_fixed is None else np.ascontiguousarray(point_fixed, np.uint8),
                      None if edge_huber is None else np.ascontiguousarray(edge_huber, np.float64),
                      None if edge_enable is None else np.ascontiguousarray(edge_enable, np.uint8)]
        a = self._keep
        fx, fy, cx, cy = cam if cam else (float(self.params.fx), float(self.params.fy), float(self.params.cx), float(self.params.cy))
        opt = lambda v, t: C.POINTER(t)() if v is None else _p(v, t)
        return BaProblem(len(a[0]), len(a[2]), len(a[3]), _p(a[0], C.c_double), _p(a[1], C.c_uint8), _p(a[2], C.c_double),
                         _p(a[3], C.c_int32), _p(a[4], C.c_int32), _p(a[5], C.c_double), fx, fy, cx, cy, float(huber_delta), formulation,
                         opt(a[6], C.c_uint8), opt(a[7], C.c_double), opt(a[8], C.c_uint8))

    @staticmethod
    def _ba_out(K, P, E):
        return dict(Hpp=np.empty((K, 6, 6)), bp=np.empty((K, 6)), Hll=np.empty((P, 3, 3)), bl=np.empty((P, 3)),
                    Hpl=np.empty((E, 6, 3)), err=np.empty((E, 2)), chi2_edge=np.empty(E), chi2=np.empty(1))

    def ba_linearize(self, poses, fixed, points, edge_pose, edge_point, obs, huber_delta=5.991, formulation=0, cam=None,
                     point_fixed=None, edge_huber=None, edge_enable=None):
        pb = self._ba_problem(poses, fixed, points, edge_pose, edge_point, obs, huber_delta, formulation, cam, point_fixed,
                              edge_huber, edge_enable)
        o = self._ba_out(pb.n_poses, pb.n_points, pb.n_edges)
        d = lambda k: _p(o[k], C.c_double)
        self._chk(self.lib.ygz_hip_ba_linearize(self._ctx, C.byref(pb), d("Hpp"), d("bp"), d("Hll"), d("bl"), d("Hpl"), d("err"),
                                                d("chi2_edge"), d("chi2")), "ba_linearize")
        o["chi2"] = float(o["chi2"][0])
        nb = C.c_int(0)
        self._chk(self.lib.ygz_hip_ba_behind_camera(self._ctx, 1023, C.byref(nb)), "ba_behind_camera")
        o["n_behind"] = nb.value
        return o

    def ceres_options(self, **kw):
        o = CeresOptions()
        self.lib.ygz_hip_ceres_default_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def ba_solve_ceres(self, poses, fixed, points, edge_pose, edge_point, obs_n, point_fixed=None, edge_huber=None,
                       edge_enable=None, options=None):
        """ceres::Solve around the GPU linearisation of a formulation-2 problem; returns (poses, points, summary dict)."""
        pb = self._ba_problem(poses, fixed, points, edge_pose, edge_point, obs_n, 0.0, 2, None, point_fixed, edge_huber, edge_enable)
        po = self._keep[0].copy()
        pt = self._keep[2].copy()
        sm = CeresSummary()
        opt = options or self.ceres_options()
        self._chk(self.lib.ygz_hip_ba_solve_ceres(self._ctx, C.byref(pb), _p(po, C.c_double), _p(pt, C.c_double), C.byref(opt),
                                                  C.byref(sm)), "ba_solve_ceres")
        return po, pt, {k: getattr(sm, k) for k, _ in CeresSummary._fields_}

    def ba_solve_ceres_resident(self, window_begin, n_windows, options=None):
        sm = (CeresSummary * n_windows)()
        opt = options or self.ceres_options()
        self._chk(self.lib.ygz_hip_ba_solve_ceres_resident(self._ctx, window_begin, n_windows, C.byref(opt), sm), "ba_solve_ceres_resident")
        return [{k: getattr(s, k) for k, _ in CeresSummary._fields_} for s in sm]

    def optimize_pose_only(self, frame_off, px, pw, poses, depth=None):
        """ba::OptimizeCurrentPoseOnly for a batch of frames; returns (poses, bad, depth, inliers, rounds)."""
        off = np.ascontiguousarray(frame_off, np.int32)
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
        pw = np.ascontiguousarray(pw, np.float64).reshape(-1, 3)
        po = np.ascontiguousarray(poses, np.float64).reshape(-1, 6).copy()
        nf, n = len(off) - 1, len(px)
        bad = np.zeros(max(n, 1), np.uint8)
        dep = np.full(max(n, 1), np.nan) if depth is None else np.ascontiguousarray(depth, np.float64).copy()
        inl, rounds = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.int32)
        self._chk(self.lib.ygz_hip_optimize_pose_only(self._ctx, nf, _p(off, C.c_int32), _p(px, C.c_double), _p(pw, C.c_double),
                                                      _p(po, C.c_double), _p(bad, C.c_uint8), _p(dep, C.c_double),
                                                      _p(inl, C.c_int32), _p(rounds, C.c_int32)), "optimize_pose_only")
        return po, bad[:n], dep[:n], inl[:nf], rounds[:nf]

    def ba_optimize(self, poses, fixed, points, edge_pose, edge_point, obs, iterations=20, huber_delta=5.991, cam=None):
        pb = self._ba_problem(poses, fixed, points, edge_pose, edge_point, obs, huber_delta, 0, cam)
        po = np.ascontiguousarray(poses, np.float64).copy()
        pt = np.ascontiguousarray(points, np.float64).copy()
        st = BaStats()
        self._chk(self.lib.ygz_hip_ba_optimize(self._ctx, C.byref(pb), _p(po, C.c_double), _p(pt, C.c_double), iterations, C.byref(st)),
                  "ba_optimize")
        return po, pt, st

    def ba_optimize_chi2(self, poses, fixed, points, edge_pose, edge_point, obs, iterations=20, huber_delta=5.991, cam=None):
        """ba_optimize + the per-edge chi2 at the optimised state (what ba::LocalBAG2O marks its outliers with): one upload, one transfer back"""
        pb = self._ba_problem(poses, fixed, points, edge_pose, edge_point, obs, huber_delta, 0, cam)
        po = np.ascontiguousarray(poses, np.float64).copy()
        pt = np.ascontiguousarray(points, np.float64).copy()
        chi = np.zeros(max(len(np.atleast_1d(edge_pose)), 1), np.float64)
        st = BaStats()
        self._chk(self.lib.ygz_hip_ba_optimize_chi2(self._ctx, C.byref(pb), _p(po, C.c_double), _p(pt, C.c_double), iterations, C.byref(st),
                                                    _p(chi, C.c_double)), "ba_optimize_chi2")
        return po, pt, st, chi[:len(np.atleast_1d(edge_pose))]

    def ba_optimize_resident(self, window_begin, n_windows, iterations=20, want_stats=True):
        st = (BaStats * n_windows)()
        self._chk(self.lib.ygz_hip_ba_optimize_resident(self._ctx, window_begin, n_windows, iterations, st if want_stats else None),
                  "ba_optimize_resident")
        return list(st) if want_stats else None

    def ba_last_path(self):
        """(resident?, reasons) of the last ba_optimize / ba_solve_ceres: the resident kernel, or the ~10x slower host loop and why"""
        v = int(self.lib.ygz_hip_ba_last_path(self._ctx))
        return bool(v & 1), [n for b, n in ((16, "more than 20 free poses"), (32, "repeated (point, pose) edges"), (64, "YGZ_BA_HOST_LOOP=1")) if v & b]

    def ba_light_barrier(self):
        """1: the same-XCD barrier of the resident LM passed its self-test on this device and is in use; 0: failed (full barriers); -1: not run yet"""
        return int(self.lib.ygz_hip_ba_light_barrier(self._ctx))

    def ba_set_team_placement(self, spread):
        self._chk(self.lib.ygz_hip_ba_set_team_placement(self._ctx, int(spread)), "ba_set_team_placement")

    def ba_set_team_budget(self, workgroups):
        self._chk(self.lib.ygz_hip_ba_set_team_budget(self._ctx, int(workgroups)), "ba_set_team_budget")

    def ba_get_state(self, window, K, P):
        po, pt = np.empty((K, 6)), np.empty((P, 3))
        self._chk(self.lib.ygz_hip_ba_get_state(self._ctx, window, _p(po, C.c_double), _p(pt, C.c_double)), "ba_get_state")
        return po, pt

    def ba_upload(self, window, poses, fixed, points, edge_pose, edge_point, obs, huber_delta=5.991, formulation=0, cam=None,
                  point_fixed=None, edge_huber=None, edge_enable=None):
        pb = self._ba_problem(poses, fixed, points, edge_pose, edge_point, obs, huber_delta, formulation, cam, point_fixed, edge_huber, edge_enable)
        self._chk(self.lib.ygz_hip_ba_upload(self._ctx, window, C.byref(pb)), "ba_upload")
        return pb.n_poses, pb.n_points, pb.n_edges

    def ba_set_enable(self, window, edge_enable):
        en = np.ascontiguousarray(edge_enable, np.uint8)
        self._chk(self.lib.ygz_hip_ba_set_enable(self._ctx, window, _p(en, C.c_uint8)), "ba_set_enable")

    def ba_set_state(self, window, poses, points):
        poses = np.ascontiguousarray(poses, np.float64)
        points = np.ascontiguousarray(points, np.float64)
        self._chk(self.lib.ygz_hip_ba_set_state(self._ctx, window, _p(poses, C.c_double), _p(points, C.c_double)), "ba_set_state")

    def ba_set_state_device(self, window, d_poses_ptr, d_points_ptr):
        self._chk(self.lib.ygz_hip_ba_set_state_device(self._ctx, window, C.c_void_p(d_poses_ptr), C.c_void_p(d_points_ptr)),
                  "ba_set_state_device")

    def ba_linearize_resident(self, window_begin=0, n_windows=1):
        self._chk(self.lib.ygz_hip_ba_linearize_resident(self._ctx, window_begin, n_windows), "ba_linearize_resident")

    def ba_download(self, window, K, P, E):
        o = self._ba_out(K, P, E)
        d = lambda k: _p(o[k], C.c_double)
        self._chk(self.lib.ygz_hip_ba_download(self._ctx, window, d("Hpp"), d("bp"), d("Hll"), d("bl"), d("Hpl"), d("err"),
                                               d("chi2_edge"), d("chi2")), "ba_download")
        o["chi2"] = float(o["chi2"][0])
        return o


class KeyframeDatabase:
    """One ygz_kfdb on a context (ygz_hip_kfdb_*): BoW vectors resident in HBM, common words and L1 scores of up to KFDB_MAX_QUERIES queries
    against every row in one launch.  Close it before its context."""

    def __init__(self, ctx):
        self.lib = ctx.lib
        kfdb_argtypes(self.lib)
        self._ctx = ctx
        self._db = C.c_void_p()
        ctx._chk(self.lib.ygz_hip_kfdb_create(ctx._ctx, C.byref(self._db)), "kfdb_create")

    def close(self):
        if self._db:
            self.lib.ygz_hip_kfdb_destroy(self._db)
        self._db = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, word, weight):
        word = np.ascontiguousarray(word, np.int32).reshape(-1)
        weight = np.ascontiguousarray(weight, np.float64).reshape(-1)
        if len(word) != len(weight):
            raise ValueError("word / weight differ in length")
        entry = C.c_int32(-1)
        self._ctx._chk(self.lib.ygz_hip_kfdb_add(self._db, _p(word, C.c_int32) if len(word) else None, _p(weight, C.c_double) if len(word) else None,
                                                 len(word), C.byref(entry)), "kfdb_add")
        return entry.value

    def erase(self, entry):
        self._ctx._chk(self.lib.ygz_hip_kfdb_erase(self._db, int(entry)), "kfdb_erase")

    def clear(self):
        self._ctx._chk(self.lib.ygz_hip_kfdb_clear(self._db), "kfdb_clear")

    def info(self):
        """(n_entries, n_alive, n_words)"""
        e, a, w = C.c_int32(), C.c_int32(), C.c_int64()
        self._ctx._chk(self.lib.ygz_hip_kfdb_info(self._db, C.byref(e), C.byref(a), C.byref(w)), "kfdb_info")
        return e.value, a.value, w.value

    def query(self, vectors):
        """vectors: a list of (word, weight); returns common [n_queries][n_entries] int32 and score [n_queries][n_entries] float64"""
        off, word, weight = kfdb_pack(vectors)
        n = self.info()[0]
        common, score = np.zeros((len(vectors), n), np.int32), np.zeros((len(vectors), n), np.float64)
        self._ctx._chk(self.lib.ygz_hip_kfdb_query(self._db, len(vectors), _p(off, C.c_int32), _p(word, C.c_int32), _p(weight, C.c_double),
                                                   _p(common, C.c_int32), _p(score, C.c_double)), "kfdb_query")
        return common, score


class ResidentMap:
    """a map that stays in device memory between calls (ygz_hip_map_*).  It belongs to its HipContext and dies with it."""

    def __init__(self, ctx):
        rmap_argtypes(ctx.lib)
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        ctx._chk(self.lib.ygz_hip_map_create(ctx._ctx, C.byref(h)), "map_create")
        self._map = h

    def destroy(self):
        if self._map is not None:
            h, self._map = self._map, None
            self.ctx._chk(self.lib.ygz_hip_map_destroy(self.ctx._ctx, h), "map_destroy")

    def info(self):
        i = MapInfo()
        self.ctx._chk(self.lib.ygz_hip_map_info(self.ctx._ctx, self._map, C.byref(i)), "map_info")
        return {name: int(getattr(i, name)) for name, _ in MapInfo._fields_}

    @staticmethod
    def pack(m):
        """the ygz_map_arrays of a dict with its keys (pt_bad and pt_has_desc optional), and the arrays that keep its pointers alive"""
        t = dict(kf_bad=np.uint8, cov=np.int32, offsets=np.int32, kf=np.int32, feat=np.int32, pt_bad=np.uint8, centre=np.float64,
                 a_offsets=np.int32, a_kf=np.int32, a_level=np.int32, pw=np.float64, pt_desc=np.uint8, pt_has_desc=np.uint8)
        ct = {np.uint8: C.c_uint8, np.int32: C.c_int32, np.float64: C.c_double}
        keep = {k: np.ascontiguousarray(m[k], t[k]) for k in t if m.get(k) is not None}
        K = len(keep["kf_bad"].reshape(-1)) if "kf_bad" in keep else int(m.get("n_keyframes", 0))
        a = MapArrays()
        a.n_keyframes = int(m.get("n_keyframes", K))
        a.n_cov = int(m.get("n_cov", keep["cov"].reshape(max(K, 1), -1).shape[1] if "cov" in keep else 0))
        a.n_points = int(m.get("n_points", len(keep["offsets"].reshape(-1)) - 1 if "offsets" in keep else 0))
        a.n_centres = int(m.get("n_centres", len(keep["centre"].reshape(-1)) // 3 if "centre" in keep else 0))
        for k in t:
            if k in keep:
                if keep[k].size == 0:
                    keep[k] = np.zeros(3, t[k])
                setattr(a, k, _p(keep[k], ct[t[k]]))
        return a, keep

    def upload(self, m, outputs=True):
        """the whole map (ygz_hip_map_upload): m is a dict with the fields of ygz_map_arrays.  dict of dmax, normal, state as the device
        computed them (outputs False: nothing comes back)"""
        a, keep = self.pack(m)
        P = max(int(a.n_points), 1)
        o = dict(dmax=np.full(P, -7.0), normal=np.full((P, 3), -7.0), state=np.full(P, -7, np.int32)) if outputs else {}
        self.ctx._chk(self.lib.ygz_hip_map_upload(self.ctx._ctx, self._map, C.byref(a), _p(o["dmax"], C.c_double) if o else None,
                                                  _p(o["normal"], C.c_double) if o else None, _p(o["state"], C.c_int32) if o else None),
                      "map_upload")
        return o

    def update(self, pt_idx=(), pw=None, pt_desc=None, pt_bad=None, pt_has_desc=None, kf_idx=(), kf_bad=None, c_idx=(), centre=None):
        """the delta after a bundle adjustment or a culling (ygz_hip_map_update); a None array keeps what the map holds"""
        arr = lambda a, t: None if a is None else np.ascontiguousarray(a, t).reshape(-1)
        pi, ki, ci = arr(pt_idx, np.int32), arr(kf_idx, np.int32), arr(c_idx, np.int32)
        x, d, b, h = arr(pw, np.float64), arr(pt_desc, np.uint8), arr(pt_bad, np.uint8), arr(pt_has_desc, np.uint8)
        kb, cc = arr(kf_bad, np.uint8), arr(centre, np.float64)
        q = lambda a, t: None if a is None or len(a) == 0 else _p(a, t)
        self.ctx._chk(self.lib.ygz_hip_map_update(self.ctx._ctx, self._map, len(pi), q(pi, C.c_int32), q(x, C.c_double), q(d, C.c_uint8),
                                                  q(b, C.c_uint8), q(h, C.c_uint8), len(ki), q(ki, C.c_int32), q(kb, C.c_uint8), len(ci),
                                                  q(ci, C.c_int32), q(cc, C.c_double)), "map_update")

    def download(self):
        """the arrays as the device holds them (ygz_hip_map_download): dict of RMAP_DOWNLOAD"""
        i = self.info()
        P, K, Kc = max(i["n_points"], 1), max(i["n_keyframes"], 1), max(i["n_centres"], 1)
        o = dict(pw=np.zeros((P, 3)), pt_desc=np.zeros((P, 32), np.uint8), pt_bad=np.zeros(P, np.uint8), pt_has_desc=np.zeros(P, np.uint8),
                 kf_bad=np.zeros(K, np.uint8), centre=np.zeros((Kc, 3)), dmax=np.zeros(P), normal=np.zeros((P, 3)), state=np.zeros(P, np.int32))
        types = {np.dtype(np.int32): C.c_int32, np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8}
        self.ctx._chk(self.lib.ygz_hip_map_download(self.ctx._ctx, self._map, *[_p(o[k], types[o[k].dtype]) for k in RMAP_DOWNLOAD]), "map_download")
        return o
