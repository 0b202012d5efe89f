// SRL -- stereo relocalisation on resident slots: ORB-SLAM2's Tracking::Relocalization up to and including its first PoseOptimization
// (SearchByBoW between a candidate keyframe and the lost frame, P3P RANSAC on the associations, the u, v, uR pose optimisation on the PnP
// inliers from the PnP pose, the first candidate that keeps enough inliers wins) for any number of lost resident frames, each with an ordered
// list of candidate keyframes, in one call.  Nothing in the reference.  The result is the composition of frozen specifications --
// yo_search_by_bow and yo_bow_orientation of oracle/bow.c, pr_ransac of tests/pnp_ref.c, tests/popt_ref.c -- joined by the formulas of
// DESIGN.md section 32 (tests/srl_ref.py); every output is bit-identical to that composition.  k_bow_transform, k_bow_match<0> (bow.hip),
// k_pnp_solve, k_pnp_score, k_pnp_select (pnp.hip) and k_pose_opt (popt.hip) are launched from here on tables, associations, sample sets and
// edges that these kernels write; problem q is (a frame, one of its candidates):
//   k_srl_gather   as k_srk_gather with a BowPair per PROBLEM: pass 0 the right columns of every distinct slot once, the count row of
//                  k_bow_transform, the pairs; pass 1, behind k_bow_transform, the masked node row of every keyframe.
//   k_srl_resolve  one workgroup per problem: the claim (integer atomicMin on the problem's int32 row), the rotation histogram in integer LDS
//                  counters, outcomes, counts, the point behind every frame keypoint, and the order-preserving compaction of the ASSOCIATIONS
//                  over keypoints: pw from the set, kx ky, uR, level.  Their number n goes to the row k_pnp_* read as the problem's end, and
//                  n < min_matches to the row that tells them to form no hypothesis.
//   k_srl_sets     lane = (problem, iteration): the three indices of pr_sample_sets(n, max_iter) from the uploaded cv::RNG words and the n
//                  that only the device knows (cvrng_dev.h).
//   k_srl_edges    one workgroup per problem, behind k_pnp_select: the PnP inlier mask back to keypoint order, the inliers compacted again
//                  into k_pose_opt's edges (none unless the PnP succeeded), the PnP pose as the optimiser's entry pose.
//   k_srl_scatter  outlier and chi2 of the edges back to keypoint order, prior = kp_point of the PnP inliers that are no optimiser outliers.
//   k_srl_pick     lane = frame: the status of each of its problems, the PnP and optimiser inlier counts, the first problem with status 0.
// FP64 in the stated order; integer atomics only; no floating-point atomic, no wait for another workgroup, no scratch, no environment switch;
// every loop is a `for` over a count known at entry; every index read from kf_point, from a match or from an association is checked before
// it addresses memory.  One packed upload, thirteen launches, one copy back, one wait.
#include "ygz_internal.h"
#include "bow_dev.h"
#include "popt_dev.h"
#include "pnp_dev.h"
#include "cvrng_dev.h"
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)
#include "ur_dev.h"
#include "slot_pose_dev.h"

using namespace ygz_pnp;

#define SL_LANES      256
#define SL_FREE       0x7fffffff         // a frame keypoint that no keyframe feature names
#define SCR_SRL       45                 // the packed block of ygz_hip_stereo_relocalize_slots; the id behind SCR_SRK, outside its enum
static_assert(SCR_SRL == SCR_SRK + 1 && SCR_SRL < YGZ_N_SCRATCH, "ygz_hip_ctx::scratch holds the id");

struct SrlSetTab { uint64_t pw; int32_t n_pt, pad_; };                  // byte offset of a set's points in the packed block

struct SrlDev {
    // the resident keypoints [max_frames][cells]
    const double *kp_px; const int32_t *kp_level; const uint32_t *kp_desc; const float *kp_angle; const int32_t *n_kp; const double *kp_depth;
    const uint8_t *kp_has_mp; const int32_t *kp_node;
    // the call: the packed block, the sets' table, the distinct slots, which slots of [slot_min, slot_min + span) the call names, the
    // keyframes (slot, set, the point behind every keypoint [n_kf][cells]), per problem its frame's slot, that slot's place in the list and
    // its keyframe, per frame where its problems begin [n_frames + 1], the cv::RNG words [3 * max_iter]
    const uint8_t *block; const SrlSetTab *set_tab;
    const int32_t *slots, *named, *kf_slot, *kf_set, *kf_point, *pr_slot, *pr_dslot, *pr_kf, *cand_off;
    const uint32_t *words;
    double *g_ur;                                    // [n_slots][cells]
    int32_t *bow_n;                                  // [span]: what k_bow_transform takes for the slots' counts
    int32_t *node1;                                  // [n_kf][cells]: the keyframe's FeatureVector nodes, -1 without a point
    BowPair *pairs; int32_t *bow_cnt;                // [P]
    // per (problem, keyframe keypoint) [P][cells]
    int32_t *match12, *outcome;
    // per (problem, frame keypoint) [P][cells]
    int32_t *holder, *kp_point, *prior, *assoc_of; uint8_t *pnp_inlier;
    // the associations of problem q: [q * cells, pnp_end[q]), what k_pnp_* read as pw, px; the mask they write
    double *a_pw, *a_px, *a_ur; int32_t *a_level, *pnp_end, *pnp_skip, *sets; const uint8_t *mask; const ygz_pnp_result *res;
    SlotEdges E;                                     // the edges of problem q: [q * cells, edge_end[q])
    int32_t *status, *counts, *rot, *best; const int32_t *inliers;
    double *poses, *T_pnp, *T_out;                   // [P][7] k_pose_opt's in and out, [P][7], [n_frames][7]
    double bf;
    int cells, n_problems, n_frames, n_slots, n_kf, slot_min, span, check_orientation, min_matches, min_final, max_iter;
};

__global__ __launch_bounds__(SL_LANES) void k_srl_gather(SrlDev A, int pass)
{
    const int y = blockIdx.y, i = blockIdx.x * SL_LANES + threadIdx.x;
    if (pass == 1) {                                                    // a keyframe's nodes, as k_bow_transform left them
        if (i >= A.cells) return;
        const int s = A.kf_slot[y];
        const bool has = i < ygz_slot_count(A.n_kp, s, A.cells) && A.kf_point[(size_t)y * A.cells + i] >= 0;
        A.node1[(size_t)y * A.cells + i] = has ? A.kp_node[(size_t)s * A.cells + i] : -1;
        return;
    }
    const int s = A.slots[y];
    if (i < ygz_slot_count(A.n_kp, s, A.cells)) {
        const size_t g = (size_t)s * A.cells + i;
        const double z = A.kp_depth[g];
        A.g_ur[(size_t)y * A.cells + i] = ygz_kp_has_depth(A.kp_has_mp[g], z) ? ygz_kp_right_column(A.kp_px[2 * g], z, A.bf) : -1.0;
    }
    if (y != 0) return;
    if (i < A.span) A.bow_n[i] = A.named[i] ? ygz_slot_count(A.n_kp, A.slot_min + i, A.cells) : 0;
    if (i < A.n_problems) {
        const int k = A.pr_kf[i], s1 = A.kf_slot[k], s2 = A.pr_slot[i];
        const size_t o1 = (size_t)s1 * A.cells, o2 = (size_t)s2 * A.cells;
        BowPair P;
        P.d1 = A.kp_desc + 8 * o1; P.d2 = A.kp_desc + 8 * o2; P.n1 = A.node1 + (size_t)k * A.cells; P.n2 = A.kp_node + o2;
        P.p1 = A.kp_px + 2 * o1; P.p2 = A.kp_px + 2 * o2; P.c1 = ygz_slot_count(A.n_kp, s1, A.cells); P.c2 = ygz_slot_count(A.n_kp, s2, A.cells);
#pragma unroll
        for (int e = 0; e < 9; ++e) P.E[e] = 0.0;
        A.pairs[i] = P;
        A.bow_cnt[i] = 0;
    }
}

enum { SL_N_UR = 0, SL_N_POINT, SL_N_MATCH, SL_N_LOST, SL_N_ROT, SL_N_COUNTERS };

__global__ __launch_bounds__(SL_LANES) void k_srl_resolve(SrlDev A)
{
    __shared__ int s_hist[30], s_ind[3], s_cnt[SL_N_COUNTERS], s_wave[SL_LANES / 64];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int k = A.pr_kf[q], s1 = A.kf_slot[k], s2 = A.pr_slot[q];
    const int cells = A.cells, n1 = ygz_slot_count(A.n_kp, s1, A.cells), n2 = ygz_slot_count(A.n_kp, s2, A.cells);
    const SrlSetTab S = A.set_tab[A.kf_set[k]];
    const int n_pt = S.n_pt;
    const double *pw = reinterpret_cast<const double *>(A.block + S.pw);
    const size_t kb = (size_t)q * cells, o1 = (size_t)s1 * cells, o2 = (size_t)s2 * cells;
    const int32_t *kfp = A.kf_point + (size_t)k * cells;
    const double *ur = A.g_ur + (size_t)A.pr_dslot[q] * cells;
    int32_t *m12 = A.match12 + kb, *holder = A.holder + kb;

    if (tid < 30) s_hist[tid] = 0;
    if (tid < 3) s_ind[tid] = -1;
    if (tid < SL_N_COUNTERS) s_cnt[tid] = 0;
    // ---- every frame keypoint is free; those with a right column
    int c_ur = 0;
    for (int j0 = 0; j0 < cells; j0 += SL_LANES) {
        const int j = j0 + tid;
        if (j < cells) holder[j] = SL_FREE;
        if (j < n2) c_ur += ur[j] >= 0 ? 1 : 0;
    }
    __syncthreads();

    // ---- the claim: frame keypoint j goes to the smallest i that names it (k_bow_match wrote m12[i] for every i < n1)
    int c_pt = 0, c_match = 0;
    for (int i0 = 0; i0 < n1; i0 += SL_LANES) {
        const int i = i0 + tid;
        if (i >= n1) continue;
        const bool has = kfp[i] >= 0;
        const int m = m12[i];
        c_pt += has ? 1 : 0;
        if (has && m >= 0 && m < n2) { ++c_match; atomicMin(&holder[m], i); }
    }
    __syncthreads();

    // ---- the rotation histogram of the claimed matches and its three maxima
    if (A.check_orientation) {
        for (int i0 = 0; i0 < n1; i0 += SL_LANES) {
            const int i = i0 + tid;
            if (i >= n1 || kfp[i] < 0) continue;
            const int m = m12[i];
            if (m < 0 || m >= n2 || holder[m] != i) continue;
            const int bin = ygz_rot_bin(A.kp_angle[o1 + i], A.kp_angle[o2 + m]);
            if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        }
        __syncthreads();
        if (tid == 0) ygz_rot_top3(s_hist, s_ind);
        __syncthreads();
    }
    const int b0 = s_ind[0], b1 = s_ind[1], b2 = s_ind[2];

    // ---- the outcome of every keyframe keypoint; a lane reads and writes its own entry of m12, and the holders stand
    int c_lost = 0, c_rot = 0;
    for (int i0 = 0; i0 < cells; i0 += SL_LANES) {
        const int i = i0 + tid;
        if (i >= cells) continue;
        int m = -1, oc = -1;
        if (i < n1 && kfp[i] >= 0) {
            const int r = m12[i];
            if (r < 0 || r >= n2) oc = 1;
            else if (holder[r] != i) { oc = 2; ++c_lost; }
            else {
                const int bin = A.check_orientation ? ygz_rot_bin(A.kp_angle[o1 + i], A.kp_angle[o2 + r]) : 0;
                if (A.check_orientation && !(bin >= 0 && (bin == b0 || bin == b1 || bin == b2))) { oc = 4; ++c_rot; }
                else { oc = 0; m = r; }
            }
        }
        m12[i] = m; A.outcome[kb + i] = oc;
    }
    if (c_ur) atomicAdd(&s_cnt[SL_N_UR], c_ur);
    if (c_pt) atomicAdd(&s_cnt[SL_N_POINT], c_pt);
    if (c_match) atomicAdd(&s_cnt[SL_N_MATCH], c_match);
    if (c_lost) atomicAdd(&s_cnt[SL_N_LOST], c_lost);
    if (c_rot) atomicAdd(&s_cnt[SL_N_ROT], c_rot);
    __syncthreads();                                                     // the counters, and the outcomes as their lanes left them
    if (tid == 0) {
        int32_t *c = A.counts + 10 * (size_t)q;
        c[0] = n1; c[1] = s_cnt[SL_N_POINT]; c[2] = n2; c[3] = s_cnt[SL_N_UR]; c[4] = s_cnt[SL_N_MATCH]; c[5] = s_cnt[SL_N_LOST];
        c[6] = s_cnt[SL_N_ROT]; c[7] = s_cnt[SL_N_MATCH] - s_cnt[SL_N_LOST] - s_cnt[SL_N_ROT];
    }
    if (tid < 33) A.rot[33 * (size_t)q + tid] = tid < 30 ? s_hist[tid] : s_ind[tid - 30];

    // ---- the point behind every frame keypoint, and the associations in keypoint order
    int running = 0;
    for (int j0 = 0; j0 < cells; j0 += SL_LANES) {
        const int j = j0 + tid;
        int p = -1;
        if (j < n2) {
            const int i = holder[j];
            if (i >= 0 && i < n1 && A.outcome[kb + i] == 0) p = kfp[i];
        }
        if (j < cells) A.kp_point[kb + j] = p;
        const bool has = p >= 0 && p < n_pt;
        const int e = ygz_edge_slot<SL_LANES>(has, running, s_wave);
        if (has) {
            const size_t ga = kb + e;
            A.a_pw[3 * ga] = pw[3 * (size_t)p]; A.a_pw[3 * ga + 1] = pw[3 * (size_t)p + 1]; A.a_pw[3 * ga + 2] = pw[3 * (size_t)p + 2];
            A.a_px[2 * ga] = A.kp_px[2 * (o2 + j)]; A.a_px[2 * ga + 1] = A.kp_px[2 * (o2 + j) + 1];
            A.a_ur[ga] = ur[j]; A.a_level[ga] = A.kp_level[o2 + j];
            A.assoc_of[kb + j] = e;
        } else if (j < cells) A.assoc_of[kb + j] = -1;
        __syncthreads();
    }
    if (tid == 0) {                                                      // running <= cells: a keypoint has at most one association
        A.pnp_end[q] = (int32_t)kb + running;
        A.pnp_skip[q] = running < A.min_matches ? 1 : 0;
    }
}

// grid (max_iter / 256, problems)
__global__ __launch_bounds__(SL_LANES) void k_srl_sets(SrlDev A)
{
    const int q = blockIdx.y, it = blockIdx.x * SL_LANES + threadIdx.x;
    if (it >= A.max_iter) return;
    const int n = A.pnp_end[q] - q * A.cells;
    int32_t s[3] = { 0, 0, 0 };                                          // a problem without PnP: its sets are not read
    if (!A.pnp_skip[q] && n >= 3) ygz_cvrng_set3(A.words[3 * it], A.words[3 * it + 1], A.words[3 * it + 2], n, s);
    int32_t *o = A.sets + ((size_t)q * A.max_iter + it) * 3;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
}

__global__ __launch_bounds__(SL_LANES) void k_srl_edges(SrlDev A)
{
    __shared__ int s_wave[SL_LANES / 64];
    const int q = blockIdx.x, tid = threadIdx.x, cells = A.cells;
    const size_t kb = (size_t)q * cells;
    const int n = A.pnp_end[q] - (int32_t)kb;
    const bool ok = !A.pnp_skip[q] && A.res[q].success != 0;           // the same in every lane
    int running = 0;
    for (int j0 = 0; j0 < cells; j0 += SL_LANES) {
        const int j = j0 + tid;
        const int a = j < cells ? A.assoc_of[kb + j] : -1;
        const bool in = a >= 0 && a < n && a < cells && A.mask[kb + a] != 0;
        if (j < cells) A.pnp_inlier[kb + j] = in ? 1 : 0;
        const bool has = ok && in;
        const int e = ygz_edge_slot<SL_LANES>(has, running, s_wave);
        if (has) {
            ygz_edge_write(A.E, kb + e, A.a_pw + 3 * (kb + a), A.a_px + 2 * (kb + a), A.a_ur[kb + a], A.a_level[kb + a]);
            A.E.edge_of[kb + j] = e;
        } else if (j < cells) A.E.edge_of[kb + j] = -1;
        __syncthreads();
    }
    if (tid == 0) A.E.edge_end[q] = (int32_t)kb + running;
    if (tid < 7) {
        const double v = A.res[q].T_cw[tid];
        A.T_pnp[7 * (size_t)q + tid] = v; A.poses[7 * (size_t)q + tid] = v;
    }
}

__global__ __launch_bounds__(SL_LANES) void k_srl_scatter(SrlDev A)
{
    const int q = blockIdx.y, j = blockIdx.x * SL_LANES + threadIdx.x;
    if (j >= A.cells) return;
    const size_t kb = (size_t)q * A.cells, g = kb + j;
    const uint8_t out = ygz_edge_scatter(A.E, kb, g, A.cells);
    A.prior[g] = A.pnp_inlier[g] && !out ? A.kp_point[g] : -1;
}

__global__ __launch_bounds__(SL_LANES) void k_srl_pick(SrlDev A)
{
    const int f = blockIdx.x * SL_LANES + threadIdx.x;
    if (f >= A.n_frames) return;
    const int q0 = A.cand_off[f], q1 = A.cand_off[f + 1];               // checked by the host: 0 <= q0 <= q1 <= n_problems
    int best = -1;
    for (int q = q0; q < q1; ++q) {
        const int pnp_in = A.res[q].n_inliers, opt_in = A.inliers[q];
        int st = 0;
        if (A.pnp_skip[q]) st = 1;
        else if (A.res[q].success == 0) st = 2;
        else if (opt_in < A.min_final) st = 3;
        A.status[q] = st;
        A.counts[10 * (size_t)q + 8] = pnp_in; A.counts[10 * (size_t)q + 9] = opt_in;
        if (st == 0 && best < 0) best = q;
    }
    A.best[f] = best;
#pragma unroll
    for (int e = 0; e < 7; ++e) A.T_out[7 * (size_t)f + e] = best >= 0 ? A.poses[7 * (size_t)best + e] : (e == 3 ? 1.0 : 0.0);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

void ygz_hip_default_srl_params(ygz_srl_params *p)
{
    if (!p) return;
    p->baseline = 0.1; p->th_low = 50; p->knn_ratio = 0.75f; p->levelsup = 4; p->check_orientation = 1; p->min_matches = 15;
    ygz_hip_default_pnp_params(&p->pnp);
    p->min_final_inliers = 50; p->pad0 = 0; p->pad1 = 0;
    ygz_hip_default_pose_opt_params(&p->pose);
    p->pose.baseline = p->baseline;
}

int ygz_hip_stereo_relocalize_slots(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_keyframes, const int32_t *kf_slot,
                                    const int32_t *kf_set, const int32_t *kf_point, int n_frames, const int32_t *slot, const int32_t *cand_off,
                                    const int32_t *cand_kf, const ygz_srl_params *params, double *T_out, int32_t *best, int32_t *status,
                                    double *T_pnp, double *T_opt, ygz_pnp_result *pnp, int32_t *counts, int32_t *inliers, int32_t *rounds_run,
                                    int32_t *round_status, int32_t *round_iterations, double *round_cost_initial, double *round_cost_final,
                                    double *round_lambda, int32_t *rot, int32_t *kp_point, uint8_t *pnp_inlier, int32_t *prior, uint8_t *outlier,
                                    double *chi2, int32_t *match12, int32_t *outcome, int32_t *sets_out)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!sets || !kf_slot || !kf_set || !kf_point || !slot || !cand_off || !cand_kf || !T_out || !best || n_sets < 1 || n_keyframes < 1 ||
        n_frames < 1)
        return YGZ_E_INVALID;
    if (n_sets > YGZ_SRL_MAX_SETS || n_keyframes > YGZ_SRL_MAX_KEYFRAMES || n_frames > YGZ_SRL_MAX_FRAMES) return YGZ_E_CAPACITY;
    if (cand_off[0] != 0) return YGZ_E_INVALID;
    for (int f = 0; f < n_frames; ++f)
        if (cand_off[f + 1] < cand_off[f]) return YGZ_E_INVALID;
    const int Pn = cand_off[n_frames];
    if (Pn < 1) return YGZ_E_INVALID;
    if (Pn > YGZ_SRL_MAX_PROBLEMS) return YGZ_E_CAPACITY;
    ygz_srl_params p;
    if (params) p = *params; else ygz_hip_default_srl_params(&p);
    if (!isfinite(p.baseline) || !isfinite(p.knn_ratio) || !isfinite(p.pnp.chi2)) return YGZ_E_INVALID;
    if (!(p.baseline > 0) || p.th_low < 0 || p.th_low > 256 || !(p.knn_ratio > 0) || p.levelsup < 0 || p.min_matches < 4 || p.min_final_inliers < 0)
        return YGZ_E_INVALID;
    if (p.pnp.max_iter < 1 || p.pnp.max_iter > YGZ_PNP_MAX_ITER || !(p.pnp.chi2 > 0) || p.pnp.min_inliers < 0) return YGZ_E_INVALID;
    if (!ygz_pose_params_ok(p.pose)) return YGZ_E_INVALID;
    if ((size_t)Pn * (size_t)p.pnp.max_iter > YGZ_SRL_MAX_HYPOTHESIS_SETS) return YGZ_E_CAPACITY;
    for (int s = 0; s < n_sets; ++s)
        if (sets[s].n_pt < 0 || (sets[s].n_pt > 0 && !sets[s].pw)) return YGZ_E_INVALID;
    for (int k = 0; k < n_keyframes; ++k)
        if (kf_slot[k] < 0 || kf_set[k] < 0 || kf_set[k] >= n_sets) return YGZ_E_INVALID;
    for (int f = 0; f < n_frames; ++f)
        if (slot[f] < 0) return YGZ_E_INVALID;
    for (int q = 0; q < Pn; ++q)
        if (cand_kf[q] < 0 || cand_kf[q] >= n_keyframes) return YGZ_E_INVALID;
    for (int s = 0; s < n_sets; ++s)
        if (sets[s].n_pt > 0 && !ygz_all_finite(sets[s].pw, 3 * (size_t)sets[s].n_pt)) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    for (int k = 0; k < n_keyframes; ++k)
        if (kf_slot[k] >= ctx->prm.max_frames) return YGZ_E_INVALID;
    for (int f = 0; f < n_frames; ++f)
        if (slot[f] >= ctx->prm.max_frames) return YGZ_E_INVALID;
    const int L = ctx->prm.pyramid_levels;
    if (L < 1 || L > YGZ_MAX_LEVELS) return YGZ_E_INVALID;
    if (ctx->cells > YGZ_SLOT_MAX_CELLS) return YGZ_E_CAPACITY;
    const size_t F = (size_t)n_frames, Kn = (size_t)n_keyframes, P = (size_t)Pn;
    const size_t Cn = (size_t)ctx->cells, NK = P * Cn;
    if (NK > (size_t)0x7fffffff) return YGZ_E_CAPACITY;                  // the rows of a problem begin at an int32
    for (size_t k = 0; k < Kn; ++k) {
        const int32_t n = sets[kf_set[k]].n_pt, *row = kf_point + k * Cn;
        for (size_t i = 0; i < Cn; ++i)
            if (row[i] < -1 || row[i] >= n) return YGZ_E_INVALID;
    }
    if (!ctx->vocab) return YGZ_E_STATE;
    for (int k = 0; k < n_keyframes; ++k)
        if (!ctx->pyr_valid[kf_slot[k]]) return YGZ_E_STATE;
    for (int f = 0; f < n_frames; ++f)
        if (!ctx->pyr_valid[slot[f]]) return YGZ_E_STATE;
    if (!ctx->kp_depth || !ctx->kp_has_mp) return YGZ_E_STATE;
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }

    // the distinct slots of the call, keyframes first, in the order they first appear; the span of slots k_bow_transform is launched over;
    // per problem its frame's slot, that slot's place among the distinct ones, and where its rows begin
    std::vector<int32_t> slots, where((size_t)ctx->prm.max_frames, -1), ps(P), ds(P), e_off(P);
    for (size_t k = 0; k < Kn; ++k) ygz_distinct_slot(slots, where, kf_slot[k]);
    for (size_t f = 0; f < F; ++f) {
        const int32_t d = ygz_distinct_slot(slots, where, slot[f]);
        for (int32_t q = cand_off[f]; q < cand_off[f + 1]; ++q) { ps[(size_t)q] = slot[f]; ds[(size_t)q] = d; }
    }
    for (size_t q = 0; q < P; ++q) e_off[q] = (int32_t)(q * Cn);
    int32_t slot_min = slots[0], slot_max = slots[0];
    for (int32_t s : slots) { if (s < slot_min) slot_min = s; if (s > slot_max) slot_max = s; }
    const size_t D = slots.size(), SP = (size_t)(slot_max - slot_min + 1);
    std::vector<int32_t> named(SP, 0);
    for (int32_t s : slots) named[(size_t)(s - slot_min)] = 1;
    const int it = p.pnp.max_iter;
    const size_t Hn = P * (size_t)it;                                    // hypothesis sets
    std::vector<uint32_t> words(3 * (size_t)it);
    ygz_cvrng_words(3 * it, words.data());

    // up: [the tables | the sets | kf_point), back: [poses | the small outputs | the per-keypoint outputs), then what stays on the device
    YgzBlobLayout B;
    const size_t o_slots = B.add_n<int32_t>(D), o_named = B.add_n<int32_t>(SP), o_kslot = B.add_n<int32_t>(Kn), o_kset = B.add_n<int32_t>(Kn);
    const size_t o_pslot = B.add_n<int32_t>(P), o_pds = B.add_n<int32_t>(P), o_pkf = B.add_n<int32_t>(P), o_off = B.add_n<int32_t>(P);
    const size_t o_coff = B.add_n<int32_t>(F + 1), o_words = B.add_n<uint32_t>(3 * (size_t)it), o_in = B.add(sizeof(PnpIn));
    const size_t o_tab = B.add_n<SrlSetTab>((size_t)n_sets);
    std::vector<SrlSetTab> tab((size_t)n_sets);
    for (int s = 0; s < n_sets; ++s) {
        tab[(size_t)s].pw = B.add_n<double>((size_t)sets[s].n_pt * 3);
        tab[(size_t)s].n_pt = sets[s].n_pt; tab[(size_t)s].pad_ = 0;
    }
    const size_t o_kfp = B.add_n<int32_t>(Kn * Cn), in_end = B.end;
    const size_t o_tout = B.add_n<double>(F * 7), o_best = B.add_n<int32_t>(F), o_status = B.add_n<int32_t>(P);
    const size_t o_tpnp = B.add_n<double>(P * 7), o_pose = B.add_n<double>(P * 7), o_res = B.add_n<ygz_pnp_result>(P);
    const size_t o_counts = B.add_n<int32_t>(P * 10);
    YgzPoseBlock PB;
    PB.add_results(B, P);
    const size_t o_rot = B.add_n<int32_t>(P * 33);
    size_t back_end = B.end;
    // the per-keypoint outputs, fetched up to the last one the caller asked for
    const size_t o_prior = B.add_n<int32_t>(NK); if (prior) back_end = B.end;
    const size_t o_kpt = B.add_n<int32_t>(NK); if (kp_point) back_end = B.end;
    const size_t o_pin = B.add_n<uint8_t>(NK); if (pnp_inlier) back_end = B.end;
    const size_t o_out = B.add_n<uint8_t>(NK); if (outlier) back_end = B.end;
    const size_t o_chi2 = B.add_n<double>(NK); if (chi2) back_end = B.end;
    const size_t o_m12 = B.add_n<int32_t>(NK); if (match12) back_end = B.end;
    const size_t o_oc = B.add_n<int32_t>(NK); if (outcome) back_end = B.end;
    const size_t o_sets = B.add_n<int32_t>(Hn * 3); if (sets_out) back_end = B.end;
    const size_t o_hold = B.add_n<int32_t>(NK), o_aof = B.add_n<int32_t>(NK);
    const size_t o_apw = B.add_n<double>(NK * 3), o_apx = B.add_n<double>(NK * 2), o_aur = B.add_n<double>(NK), o_alv = B.add_n<int32_t>(NK);
    const size_t o_mask = B.add_n<uint8_t>(NK), o_pend = B.add_n<int32_t>(P), o_skip = B.add_n<int32_t>(P);
    PB.add_edges(B, P, Cn);
    const size_t o_gur = B.add_n<double>(D * Cn), o_bown = B.add_n<int32_t>(SP), o_node1 = B.add_n<int32_t>(Kn * Cn);
    const size_t o_pairs = B.add_n<BowPair>(P), o_bcnt = B.add_n<int32_t>(P);
    const size_t o_nsol = B.add_n<int32_t>(Hn), o_hcnt = B.add_n<int32_t>(Hn * 4), o_sol = B.add_n<double>(Hn * 48), total = B.end;
    YgzBlob blob;
    int rc = ygz_blob_open(ctx, SCR_SRL, total, back_end, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    const ygz_hip_ctx::Vocab *v = ctx->vocab;
    const double K4[4] = { (double)ctx->prm.fx, (double)ctx->prm.fy, (double)ctx->prm.cx, (double)ctx->prm.cy };
    PnpIn in;
    memset(&in, 0, sizeof in);
    for (int k = 0; k < 4; ++k) in.K4[k] = K4[k];
    in.chi2 = p.pnp.chi2; in.n_problems = Pn; in.max_iter = it; in.min_inliers = p.pnp.min_inliers;
    memcpy(up + o_slots, slots.data(), D * 4); memcpy(up + o_named, named.data(), SP * 4);
    memcpy(up + o_kslot, kf_slot, Kn * 4); memcpy(up + o_kset, kf_set, Kn * 4);
    memcpy(up + o_pslot, ps.data(), P * 4); memcpy(up + o_pds, ds.data(), P * 4); memcpy(up + o_pkf, cand_kf, P * 4);
    memcpy(up + o_off, e_off.data(), P * 4); memcpy(up + o_coff, cand_off, (F + 1) * 4);
    memcpy(up + o_words, words.data(), words.size() * 4); memcpy(up + o_in, &in, sizeof in);
    memcpy(up + o_tab, tab.data(), (size_t)n_sets * sizeof(SrlSetTab));
    for (int s = 0; s < n_sets; ++s)
        if (sets[s].n_pt > 0) memcpy(up + tab[(size_t)s].pw, sets[s].pw, (size_t)sets[s].n_pt * 24);
    memcpy(up + o_kfp, kf_point, Kn * Cn * 4);
    if ((rc = ygz_blob_upload(ctx, blob, in_end)) != YGZ_OK) return rc;

    SrlDev A;
    memset(&A, 0, sizeof A);
    A.kp_px = ctx->kp_px; A.kp_level = ctx->kp_level; A.kp_desc = ctx->kp_desc; A.kp_angle = ctx->kp_angle; A.n_kp = ctx->n_kp;
    A.kp_depth = ctx->kp_depth; A.kp_has_mp = ctx->kp_has_mp; A.kp_node = v->kp_node;
    A.block = dev; A.set_tab = ygz_at<const SrlSetTab>(dev, o_tab);
    A.slots = ygz_at<const int32_t>(dev, o_slots); A.named = ygz_at<const int32_t>(dev, o_named);
    A.kf_slot = ygz_at<const int32_t>(dev, o_kslot); A.kf_set = ygz_at<const int32_t>(dev, o_kset); A.kf_point = ygz_at<const int32_t>(dev, o_kfp);
    A.pr_slot = ygz_at<const int32_t>(dev, o_pslot); A.pr_dslot = ygz_at<const int32_t>(dev, o_pds); A.pr_kf = ygz_at<const int32_t>(dev, o_pkf);
    A.cand_off = ygz_at<const int32_t>(dev, o_coff); A.words = ygz_at<const uint32_t>(dev, o_words);
    A.g_ur = ygz_at<double>(dev, o_gur); A.bow_n = ygz_at<int32_t>(dev, o_bown); A.node1 = ygz_at<int32_t>(dev, o_node1);
    A.pairs = ygz_at<BowPair>(dev, o_pairs); A.bow_cnt = ygz_at<int32_t>(dev, o_bcnt);
    A.match12 = ygz_at<int32_t>(dev, o_m12); A.outcome = ygz_at<int32_t>(dev, o_oc);
    A.holder = ygz_at<int32_t>(dev, o_hold); A.kp_point = ygz_at<int32_t>(dev, o_kpt); A.prior = ygz_at<int32_t>(dev, o_prior);
    A.assoc_of = ygz_at<int32_t>(dev, o_aof); A.pnp_inlier = dev + o_pin;
    A.a_pw = ygz_at<double>(dev, o_apw); A.a_px = ygz_at<double>(dev, o_apx); A.a_ur = ygz_at<double>(dev, o_aur);
    A.a_level = ygz_at<int32_t>(dev, o_alv); A.pnp_end = ygz_at<int32_t>(dev, o_pend); A.pnp_skip = ygz_at<int32_t>(dev, o_skip);
    A.sets = ygz_at<int32_t>(dev, o_sets); A.mask = dev + o_mask; A.res = ygz_at<const ygz_pnp_result>(dev, o_res);
    ygz_slot_edges_bind(A.E, dev, PB, o_out, o_chi2);
    A.status = ygz_at<int32_t>(dev, o_status); A.counts = ygz_at<int32_t>(dev, o_counts); A.rot = ygz_at<int32_t>(dev, o_rot);
    A.best = ygz_at<int32_t>(dev, o_best); A.inliers = ygz_at<const int32_t>(dev, PB.inliers);
    A.poses = ygz_at<double>(dev, o_pose); A.T_pnp = ygz_at<double>(dev, o_tpnp); A.T_out = ygz_at<double>(dev, o_tout);
    A.bf = K4[0] * p.baseline;
    A.cells = ctx->cells; A.n_problems = Pn; A.n_frames = n_frames; A.n_slots = (int)D; A.n_kf = n_keyframes; A.slot_min = slot_min;
    A.span = (int)SP; A.check_orientation = p.check_orientation ? 1 : 0; A.min_matches = p.min_matches; A.min_final = p.min_final_inliers;
    A.max_iter = it;

    VocDev V;
    V.L = v->L; V.child_off = v->child_off; V.child = v->child; V.word_id = v->word_id; V.desc = v->desc; V.weight = v->weight;

    PnpDev Q;
    Q.in = ygz_at<const PnpIn>(dev, o_in); Q.off = ygz_at<const int32_t>(dev, o_off); Q.pw = A.a_pw; Q.px = A.a_px; Q.sets = A.sets;
    Q.res = ygz_at<ygz_pnp_result>(dev, o_res); Q.mask = dev + o_mask; Q.nsol = ygz_at<int32_t>(dev, o_nsol);
    Q.counts = ygz_at<int32_t>(dev, o_hcnt); Q.sol = ygz_at<double>(dev, o_sol); Q.end = A.pnp_end; Q.skip = A.pnp_skip;

    PoptArgs G;
    memset(&G, 0, sizeof G);
    ygz_popt_bind(G, dev, PB, o_off, o_pose);
    ygz_popt_set_params(G, K4, p.baseline, p.pose);

    int widest = ctx->cells > Pn ? ctx->cells : Pn;
    if ((int)SP > widest) widest = (int)SP;
    const unsigned bx = (unsigned)ygz_div_up(ctx->cells, SL_LANES), bt = (unsigned)ygz_div_up(widest, SL_LANES), np = (unsigned)Pn;
    const size_t so = (size_t)slot_min * Cn;
    YGZ_LAUNCH(ctx, KID_SRL_GATHER, k_srl_gather, dim3(bt, (unsigned)D), dim3(SL_LANES), A, 0);
    YGZ_LAUNCH(ctx, KID_BOW_TRANSFORM, k_bow_transform, dim3(bx, (unsigned)SP), dim3(256), V, ctx->kp_desc + 8 * so, (const int32_t *)A.bow_n, 0, Cn,
               p.levelsup, v->kp_word + so, v->kp_weight + so, v->kp_node + so);
    YGZ_LAUNCH(ctx, KID_SRL_GATHER, k_srl_gather, dim3(bx, (unsigned)n_keyframes), dim3(SL_LANES), A, 1);
    YGZ_LAUNCH(ctx, KID_BOW_MATCH, k_bow_match<0>, dim3(bx, np), dim3(256), (const BowPair *)A.pairs, (int)p.th_low, p.knn_ratio, 0.0,
               K4[0], K4[1], K4[2], K4[3], A.match12, Cn, A.bow_cnt);
    YGZ_LAUNCH(ctx, KID_SRL_RESOLVE, k_srl_resolve, dim3(np), dim3(SL_LANES), A);
    YGZ_LAUNCH(ctx, KID_SRL_SETS, k_srl_sets, dim3((unsigned)ygz_div_up(it, SL_LANES), np), dim3(SL_LANES), A);
    YGZ_LAUNCH(ctx, KID_PNP_SOLVE, k_pnp_solve, dim3((unsigned)ygz_div_up(it, PNP_SOLVE_LANES), np), dim3(PNP_SOLVE_LANES), Q);
    YGZ_LAUNCH(ctx, KID_PNP_SCORE, k_pnp_score, dim3((unsigned)ygz_div_up(4 * it, PNP_SCORE_LANES), np), dim3(PNP_SCORE_LANES), Q);
    YGZ_LAUNCH(ctx, KID_PNP_SELECT, k_pnp_select, dim3(np), dim3(PNP_SEL_THREADS), Q);
    YGZ_LAUNCH(ctx, KID_SRL_EDGES, k_srl_edges, dim3(np), dim3(SL_LANES), A);
    YGZ_LAUNCH(ctx, KID_POSE_OPT, k_pose_opt, dim3(np), dim3(PT_DEV_THREADS), G);
    YGZ_LAUNCH(ctx, KID_SRL_SCATTER, k_srl_scatter, dim3(bx, np), dim3(SL_LANES), A);
    YGZ_LAUNCH(ctx, KID_SRL_PICK, k_srl_pick, dim3((unsigned)ygz_div_up(n_frames, SL_LANES)), dim3(SL_LANES), A);
    if ((rc = ygz_blob_fetch(ctx, blob, o_tout, back_end)) != YGZ_OK) return rc;
    memcpy(T_out, up + o_tout, F * 56);
    memcpy(best, up + o_best, F * 4);
    if (status) memcpy(status, up + o_status, P * 4);
    if (T_pnp) memcpy(T_pnp, up + o_tpnp, P * 56);
    if (T_opt) memcpy(T_opt, up + o_pose, P * 56);
    if (pnp) memcpy(pnp, up + o_res, P * sizeof(ygz_pnp_result));
    if (counts) memcpy(counts, up + o_counts, P * 40);
    PB.copy_results(up, P, inliers, rounds_run, round_status, round_iterations, round_cost_initial, round_cost_final, round_lambda);
    if (rot) memcpy(rot, up + o_rot, P * 132);
    if (prior) memcpy(prior, up + o_prior, NK * 4);
    if (kp_point) memcpy(kp_point, up + o_kpt, NK * 4);
    if (pnp_inlier) memcpy(pnp_inlier, up + o_pin, NK);
    if (outlier) memcpy(outlier, up + o_out, NK);
    if (chi2) memcpy(chi2, up + o_chi2, NK * 8);
    if (match12) memcpy(match12, up + o_m12, NK * 4);
    if (outcome) memcpy(outcome, up + o_oc, NK * 4);
    if (sets_out) memcpy(sets_out, up + o_sets, Hn * 12);
    return YGZ_OK;
}

}  // extern "C"
