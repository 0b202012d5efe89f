// Stereo local-map tracking on an indexed map: ygz_hip_stereo_local_map_slots with the point sets given as index lists
// into ONE map, in the layout ygz_hip_local_map_select writes (local_pt, n_pt).  The host body is slm.hip's, shared through slm_share.h; this
// file adds the source of the sets:
//   k_slm_index   grid (ceil(longest list / 256), lists), lane = one entry of one list: the 88 bytes of map point list_pt[l][i] (pw, the
//                 descriptor as two 16-byte words, dmax, normal) are copied to place i of list l's packed arrays, which lie in the part of the
//                 call's block that stays on the device.  k_slm_gather and k_strack_search read them as they read uploaded sets.
// A list no frame of the call reads has length 0 in the table and is not gathered.  Plain copies: no arithmetic, no atomic, no LDS, no scratch
// memory, no environment switch; every index was validated by the entry point.
#include "slm_share.h"

namespace {

#define SLI_LANES 256

__global__ __launch_bounds__(SLI_LANES) void k_slm_index(SlmIndexDev A)
{
    const int l = (int)blockIdx.y, i = (int)blockIdx.x * SLI_LANES + (int)threadIdx.x;
    const SlmSetTab t = A.tab[l];
    if (i >= t.n_pt) return;
    const size_t p = (size_t)A.list_pt[(size_t)l * (size_t)A.stride + (size_t)i], at = (size_t)i;
    double *pw = reinterpret_cast<double *>(A.block + t.pw) + 3 * at, *normal = reinterpret_cast<double *>(A.block + t.normal) + 3 * at;
    uint4 *desc = reinterpret_cast<uint4 *>(A.block + t.desc) + 2 * at;
    pw[0] = A.pw[3 * p]; pw[1] = A.pw[3 * p + 1]; pw[2] = A.pw[3 * p + 2];
    desc[0] = A.desc[2 * p]; desc[1] = A.desc[2 * p + 1];
    reinterpret_cast<double *>(A.block + t.dmax)[at] = A.dmax[p];
    normal[0] = A.normal[3 * p]; normal[1] = A.normal[3 * p + 1]; normal[2] = A.normal[3 * p + 2];
}

}  // namespace

// also the `index` of the resident source (rmap.hip): there the table's lengths are written by a launch in front of this one
void ygz_slm_launch_index(ygz_hip_ctx *ctx, const SlmIndexDev &A, int n_lists, int longest)
{
    YGZ_LAUNCH(ctx, KID_SLM_INDEX, k_slm_index, dim3((unsigned)ygz_div_up(longest, SLI_LANES), (unsigned)n_lists), dim3(SLI_LANES), A);
}

extern "C" {

int ygz_hip_stereo_local_map_indexed(ygz_hip_ctx *ctx, int n_points, const double *pw, const uint8_t *pt_desc, const double *pt_dmax,
                                     const double *pt_normal, int n_lists, int list_stride, const int32_t *list_pt, const int32_t *list_len,
                                     int n_frames, const int32_t *slot, const int32_t *list, const double *T, const int32_t *prior,
                                     const ygz_slm_params *params, double *T_out, int32_t *status, int32_t *counts, int32_t *kp_point,
                                     uint8_t *outlier, double *chi2, int32_t *inliers, int32_t *rounds_run, int32_t *round_status,
                                     int32_t *round_iterations, double *round_cost_initial, double *round_cost_final, double *round_lambda,
                                     int32_t *match, int32_t *dist, int32_t *level, int32_t *reason, int32_t *outcome, int32_t *n_cand,
                                     int32_t *n_gated, double *proj)
{
    SlmSource src;
    src.n_sets = n_lists; src.n_points = n_points; src.stride = list_stride;
    src.pw = pw; src.desc = pt_desc; src.dmax = pt_dmax; src.normal = pt_normal;
    src.list_pt = list_pt; src.list_len = list_len; src.index = ygz_slm_launch_index;
    const SlmOutputs out = { T_out, status, counts, kp_point, outlier, chi2, inliers, rounds_run, round_status, round_iterations, round_cost_initial,
                             round_cost_final, round_lambda, match, dist, level, reason, outcome, n_cand, n_gated, proj };
    return ygz_slm_run(ctx, src, n_frames, slot, list, T, prior, params, out);
}

}  // extern "C"
