// SLM -- stereo local-map tracking on resident slots: ORB-SLAM2's TrackLocalMap (SearchByProjection(F, vpMapPoints, th) and the u, v, uR pose
// optimisation on the frame's own associations plus the new ones) for any number of resident frames in one call.  Nothing in the reference,
// whose tracker is monocular.  The result is the composition of two frozen specifications, tests/strack_ref.c in mode LOCAL and
// tests/popt_ref.c, joined by four formulas (tests/slm_ref.py); every output is bit-identical to that composition.
// k_strack_search (strack.hip) and k_pose_opt (popt.hip) are launched from here on tables and edges that these kernels write:
//   k_slm_gather   rows 0 .. n_slots - 1: lane = one keypoint of one DISTINCT slot of the call, kp_ur = u - bf / z once per slot; the first
//                  lanes of row 0 also write every StSetDev and every frame's StProbDev entry, n_kp from the slot's own count: the host reads
//                  no count.  Rows behind them (launched with a prior only): lane = one keypoint of one frame, kp_taken = (prior >= 0) and a
//                  plain byte store of 1 into the frame's pt_skip row, which the packed block zeroed.
//   k_slm_resolve  one workgroup per frame, built for throughput over frames.  The taken bitmap is in LDS and starts from the prior.  Of 256
//                  points at a time those with reason 0 and a non-empty list are compacted (ballot and popcount) and staged in LDS with the
//                  levels of their eight entries; lane 0 walks only those: e1, e2 the first two free entries, the distance rule, the ratio
//                  rule of LOCAL on two staged levels, the claim.  The rest is parallel: outcomes, the point every keypoint ends with, the
//                  counts, and the order-preserving compaction of the edges over KEYPOINTS with pw fetched from the set.
//   k_slm_scatter  outlier and chi2 of the edges back to keypoint order.
// FP64 in the stated order; integer atomics on LDS counters only; no floating-point atomic, no wait for another workgroup, no scratch, no
// environment switch; every loop is a `for` over a count known at entry; every index read from a key or from the prior is checked against
// n_kp / n_pt before it addresses memory.  One packed upload, five launches, one copy back, one wait.
// The host body, ygz_slm_run, also serves ygz_hip_stereo_local_map_indexed (slm_index.hip, slm_share.h): there the sets are gathered on the
// device from index lists into one map by a sixth launch in front of these five, and
// ygz_hip_stereo_local_map_resident (rmap.hip): there the map is resident, and the lists, their lengths and the prior are written by the
// launches of the source's hook, so every list has the stride as its room and its length exists on the device alone (section 36).
#include "ygz_internal.h"
#include "strack_dev.h"
#include "popt_dev.h"
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)
#include "ur_dev.h"
#include "slot_pose_dev.h"
#include "slm_share.h"

#define SL_LANES      256

struct SlmDev {
    // the resident keypoints [max_frames][cells]
    const double *kp_px; const int32_t *kp_level; const uint32_t *kp_desc; const int32_t *n_kp; const double *kp_depth; const uint8_t *kp_has_mp;
    // the call: the packed block, the sets' table, the distinct slots, per frame its slot, that slot's place in the list, its set and where
    // its points begin in the per-point arrays; the prior [n_frames][cells] or nullptr
    uint8_t *block; const SlmSetTab *set_tab;
    const int32_t *slots, *fr_slot, *fr_dslot, *fr_set, *pt_off, *prior;
    double *poses;                                   // [n_frames][7]: T in, T_out out (k_pose_opt)
    double *g_ur;                                    // [n_slots][cells]
    uint8_t *kp_taken, *pt_skip;                     // [n_frames][cells], [N]
    StSetDev *sets; StProbDev *probs;                // [n_sets], [n_frames]
    // per (frame, point), concatenated [N]
    uint32_t *keys; int32_t *n_cand, *n_gated, *level, *reason; double *proj;
    int32_t *match, *dist, *outcome;
    // per (frame, keypoint) [n_frames][cells]
    int32_t *kp_point;
    SlotEdges E;                                     // the edges of frame f: [f * cells, edge_end[f])
    int32_t *status, *counts;
    double bf, th, ratio;
    int cells, n_frames, n_slots, n_sets, th_dist, min_edges;
};

__global__ __launch_bounds__(SL_LANES) void k_slm_gather(SlmDev A)
{
    const int y = blockIdx.y, i = blockIdx.x * SL_LANES + threadIdx.x;
    if (y >= A.n_slots) {                                               // a frame's prior: its taken flags and its skip bytes
        const int f = y - A.n_slots;
        if (i >= ygz_slot_count(A.n_kp, A.fr_slot[f], A.cells)) return;
        const int pr = A.prior[(size_t)f * A.cells + i];
        A.kp_taken[(size_t)f * A.cells + i] = pr >= 0 ? 1 : 0;
        if (pr >= 0 && pr < A.set_tab[A.fr_set[f]].n_pt) A.pt_skip[(size_t)A.pt_off[f] + pr] = 1;
        return;
    }
    const int s = A.slots[y];
    if (i < ygz_slot_count(A.n_kp, s, A.cells)) {
        const size_t g = (size_t)s * A.cells + i;
        const double z = A.kp_depth[g];
        A.g_ur[(size_t)y * A.cells + i] = ygz_kp_has_depth(A.kp_has_mp[g], z) ? ygz_kp_right_column(A.kp_px[2 * g], z, A.bf) : -1.0;
    }
    if (y != 0) return;
    if (i < A.n_sets) {
        const SlmSetTab t = A.set_tab[i];
        StSetDev S;
        S.pw = reinterpret_cast<const double *>(A.block + t.pw); S.pt_desc = reinterpret_cast<const uint32_t *>(A.block + t.desc);
        S.pt_level = nullptr;
        S.pt_dmax = reinterpret_cast<const double *>(A.block + t.dmax); S.pt_normal = reinterpret_cast<const double *>(A.block + t.normal);
        S.n_pt = t.n_pt; S.pad_ = 0;
        A.sets[i] = S;
    }
    if (i < A.n_frames) {
        const int sl = A.fr_slot[i];
        const size_t o = (size_t)sl * A.cells;
        StProbDev P;
        P.kp_px = A.kp_px + 2 * o; P.kp_level = A.kp_level + o; P.kp_desc = A.kp_desc + 8 * o; P.kp_ur = A.g_ur + (size_t)A.fr_dslot[i] * A.cells;
        P.kp_taken = A.prior ? A.kp_taken + (size_t)i * A.cells : nullptr;
        P.pt_skip = A.prior ? A.pt_skip + (size_t)A.pt_off[i] : nullptr;
        P.n_kp = ygz_slot_count(A.n_kp, sl, A.cells); P.set = A.fr_set[i]; P.pt_off = A.pt_off[i]; P.mode = 1; P.direction = 0; P.pad_ = 0;
        P.th = A.th;
#pragma unroll
        for (int k = 0; k < 7; ++k) P.T[k] = A.poses[7 * (size_t)i + k];
        A.probs[i] = P;
    }
}

enum { SL_N_UR = 0, SL_N_PRIOR, SL_N_SEARCHED, SL_N_OVER, SL_N_NEW, SL_N_COUNTERS };

__global__ __launch_bounds__(SL_LANES) void k_slm_resolve(SlmDev A)
{
    __shared__ uint32_t s_taken[YGZ_SLOT_MAX_CELLS / 32];
    __shared__ uint4 s_key[SL_LANES][2];
    __shared__ uint2 s_lv[SL_LANES];                                     // the levels of a staged list's eight entries, a byte each
    __shared__ uint32_t s_pick[SL_LANES];
    __shared__ int s_oc[SL_LANES], s_cnt[SL_N_COUNTERS], s_wave[SL_LANES / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const StProbDev &P = A.probs[f];
    const StSetDev &S = A.sets[P.set];
    const int cells = A.cells, n_pt = S.n_pt, n_kp = P.n_kp;
    const size_t kb = (size_t)f * cells, pb = (size_t)P.pt_off;
    const int32_t *prior = A.prior ? A.prior + kb : nullptr;
    const uint32_t idx_mask = (1u << ST_DEV_IDX_BITS) - 1;

    if (tid < SL_N_COUNTERS) s_cnt[tid] = 0;
    // ---- the prior: the bitmap, the point a keypoint already holds (-1 past the last keypoint), the keypoints with a right column
    int c_ur = 0, c_prior = 0;
    for (int j0 = 0; j0 < cells; j0 += SL_LANES) {
        const int j = j0 + tid;
        int pr = -1;
        bool tk = false;
        if (j < n_kp) {
            if (prior) { pr = prior[j]; tk = pr >= 0; if (pr >= n_pt) pr = -1; }
            c_ur += P.kp_ur[j] >= 0 ? 1 : 0;
            c_prior += pr >= 0 ? 1 : 0;
        }
        if (j < cells) A.kp_point[kb + j] = pr;
        const unsigned long long bal = __ballot(tk);
        if (lane == 0 && j0 + wv * 64 < cells) {
            s_taken[(j0 + wv * 64) >> 5] = (uint32_t)bal;
            s_taken[((j0 + wv * 64) >> 5) + 1] = (uint32_t)(bal >> 32);
        }
    }
    __syncthreads();

    // ---- section 26's step 8 with the LOCAL rule.  A list is sorted and padded with empty entries; a point with reason != 0 or an empty list
    // claims nothing and reads no flag, so only the others are staged and walked
    int c_search = 0, c_over = 0, c_new = 0;
    for (int c0 = 0; c0 < n_pt; c0 += SL_LANES) {
        const int i = c0 + tid;
        int why = -1, nc = 0;
        uint4 a = make_uint4(ST_DEV_NO_KEY, ST_DEV_NO_KEY, ST_DEV_NO_KEY, ST_DEV_NO_KEY), b = a;
        if (i < n_pt) {
            why = A.reason[pb + i]; nc = A.n_cand[pb + i];
            const uint4 *k = reinterpret_cast<const uint4 *>(A.keys + YGZ_STRACK_TOPK * (pb + i));
            a = k[0]; b = k[1];
        }
        const bool act = why == 0 && a.x != ST_DEV_NO_KEY;
        const unsigned long long bal = __ballot(act);
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        int at = 0, total = 0;
#pragma unroll
        for (int w = 0; w < SL_LANES / 64; ++w) { const int c = s_wave[w]; if (w < wv) at += c; total += c; }
        at += __popcll(bal & ((1ull << lane) - 1ull));
        if (act) {
            s_key[at][0] = a; s_key[at][1] = b;
            // an entry that is empty or past the last keypoint is never free: its level is not read
#define SL_LV_(key) (((key) != ST_DEV_NO_KEY && ((key) & idx_mask) < (uint32_t)n_kp) ? ((uint32_t)P.kp_level[(key) & idx_mask] & 255u) : 255u)
            const uint32_t l0 = SL_LV_(a.x), l1 = SL_LV_(a.y), l2 = SL_LV_(a.z), l3 = SL_LV_(a.w);
            const uint32_t l4 = SL_LV_(b.x), l5 = SL_LV_(b.y), l6 = SL_LV_(b.z), l7 = SL_LV_(b.w);
#undef SL_LV_
            s_lv[at] = make_uint2(l0 | (l1 << 8) | (l2 << 16) | (l3 << 24), l4 | (l5 << 8) | (l6 << 16) | (l7 << 24));
        }
        __syncthreads();
        if (tid == 0) {
            for (int t = 0; t < total; ++t) {
                const uint4 ka = s_key[t][0], kc = s_key[t][1];
                const uint2 lv = s_lv[t];
                uint32_t e1 = ST_DEV_NO_KEY, e2 = ST_DEV_NO_KEY, v1 = 0, v2 = 0;
                // the reads of the bitmap are independent; the entries are tried from the last to the first, so e1 and e2 end as the first
                // two free ones
#define SL_TRY_(key, lvl) { const uint32_t k_ = (key), j_ = k_ & idx_mask;                                              \
                            const bool in_ = k_ != ST_DEV_NO_KEY && j_ < (uint32_t)n_kp;                                  \
                            const uint32_t word_ = s_taken[in_ ? (j_ >> 5) : 0];                                          \
                            if (in_ && !((word_ >> (j_ & 31)) & 1u)) { e2 = e1; v2 = v1; e1 = k_; v1 = (lvl) & 255u; } }
                SL_TRY_(kc.w, lv.y >> 24) SL_TRY_(kc.z, lv.y >> 16) SL_TRY_(kc.y, lv.y >> 8) SL_TRY_(kc.x, lv.y)
                SL_TRY_(ka.w, lv.x >> 24) SL_TRY_(ka.z, lv.x >> 16) SL_TRY_(ka.y, lv.x >> 8) SL_TRY_(ka.x, lv.x)
#undef SL_TRY_
                const int d1 = (int)(e1 >> ST_DEV_IDX_BITS), d2 = (int)(e2 >> ST_DEV_IDX_BITS);
                int oc;
                if (e1 == ST_DEV_NO_KEY) oc = 1;
                else if (d1 > A.th_dist) oc = 2;
                else if (e2 != ST_DEV_NO_KEY && v1 == v2 && (double)d1 > A.ratio * (double)d2) oc = 3;
                else { oc = 0; s_taken[(e1 & idx_mask) >> 5] |= 1u << (e1 & 31); }
                s_pick[t] = e1; s_oc[t] = oc;
            }
        }
        __syncthreads();
        if (i < n_pt) {
            int m = -1, d = -1, oc = -1;
            if (why == 0) {
                ++c_search;
                if (nc > YGZ_STRACK_TOPK) ++c_over;
                oc = act ? s_oc[at] : 1;
                if (oc == 0) {
                    const uint32_t pick = s_pick[at];
                    m = (int)(pick & idx_mask); d = (int)(pick >> ST_DEV_IDX_BITS); ++c_new;
                    A.kp_point[kb + m] = i;                              // m < n_kp: the walk checked it; no other point claims m
                }
            }
            A.match[pb + i] = m; A.dist[pb + i] = d; A.outcome[pb + i] = oc;
        }
    }
    if (c_ur) atomicAdd(&s_cnt[SL_N_UR], c_ur);
    if (c_prior) atomicAdd(&s_cnt[SL_N_PRIOR], c_prior);
    if (c_search) atomicAdd(&s_cnt[SL_N_SEARCHED], c_search);
    if (c_over) atomicAdd(&s_cnt[SL_N_OVER], c_over);
    if (c_new) atomicAdd(&s_cnt[SL_N_NEW], c_new);
    __syncthreads();                                                     // the counters, and kp_point as the claiming lanes left it
    const int n_edges = s_cnt[SL_N_PRIOR] + s_cnt[SL_N_NEW];
    const int status = n_edges < A.min_edges ? 1 : 0;                    // the same in every lane
    if (tid == 0) {
        int32_t *c = A.counts + 8 * (size_t)f;
        c[0] = n_kp; c[1] = s_cnt[SL_N_UR]; c[2] = s_cnt[SL_N_PRIOR]; c[3] = n_pt; c[4] = s_cnt[SL_N_SEARCHED]; c[5] = s_cnt[SL_N_OVER];
        c[6] = s_cnt[SL_N_NEW]; c[7] = n_edges;
        A.status[f] = status;
    }

    // ---- the edges: the keypoints with a point in keypoint order (none for a frame with too few)
    int running = 0;
    for (int j0 = 0; j0 < cells; j0 += SL_LANES) {
        const int j = j0 + tid;
        const int i = (status == 0 && j < n_kp) ? A.kp_point[kb + j] : -1;
        const bool has = i >= 0 && i < n_pt;
        const int e = ygz_edge_slot<SL_LANES>(has, running, s_wave);
        if (has) {
            ygz_edge_write(A.E, kb + e, S.pw + 3 * (size_t)i, P.kp_px + 2 * (size_t)j, P.kp_ur[j], P.kp_level[j]);
            A.E.edge_of[kb + j] = e;
        } else if (j < cells) A.E.edge_of[kb + j] = -1;
        __syncthreads();
    }
    if (tid == 0) A.E.edge_end[f] = (int32_t)kb + running;
}

__global__ __launch_bounds__(SL_LANES) void k_slm_scatter(SlmDev A)
{
    const int f = blockIdx.y, j = blockIdx.x * SL_LANES + threadIdx.x;
    if (j >= A.cells) return;
    const size_t kb = (size_t)f * A.cells;
    ygz_edge_scatter(A.E, kb, kb + j, A.cells);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

void ygz_hip_default_slm_params(ygz_slm_params *p)
{
    if (!p) return;
    p->baseline = 0.1; p->th = 1.0; p->ratio = 0.8; p->r_near = 2.5; p->r_wide = 4.0; p->cos_near = 0.998; p->th_dist = 100; p->min_edges = 3;
    ygz_hip_default_pose_opt_params(&p->pose);
    p->pose.baseline = p->baseline;
}

int ygz_hip_stereo_local_map_slots(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_frames, const int32_t *slot,
                                   const int32_t *set, const double *T, const int32_t *prior, const ygz_slm_params *params, double *T_out,
                                   int32_t *status, int32_t *counts, int32_t *kp_point, uint8_t *outlier, double *chi2, int32_t *inliers,
                                   int32_t *rounds_run, int32_t *round_status, int32_t *round_iterations, double *round_cost_initial,
                                   double *round_cost_final, double *round_lambda, int32_t *match, int32_t *dist, int32_t *level,
                                   int32_t *reason, int32_t *outcome, int32_t *n_cand, int32_t *n_gated, double *proj)
{
    SlmSource src;
    src.n_sets = n_sets; src.sets = sets;
    const SlmOutputs out = { T_out, status, counts, kp_point, outlier, chi2, inliers, rounds_run, round_status, round_iterations, round_cost_initial,
                             round_cost_final, round_lambda, match, dist, level, reason, outcome, n_cand, n_gated, proj };
    return ygz_slm_run(ctx, src, n_frames, slot, set, T, prior, params, out);
}

}  // extern "C"

// the body of ygz_hip_stereo_local_map_slots and ygz_hip_stereo_local_map_indexed (slm_share.h): `src` holds the sets, or the map and the lists
int ygz_slm_run(ygz_hip_ctx *ctx, const SlmSource &src, int n_frames, const int32_t *slot, const int32_t *set, const double *T,
                const int32_t *prior, const ygz_slm_params *params, const SlmOutputs &out)
{
    const bool indexed = src.indexed(), resident = src.is_resident();   // resident is indexed with the map, the lists and the prior on the device
    const int n_sets = src.n_sets;
    const ygz_strack_points *sets = src.sets;
    double *T_out = out.T_out, *chi2 = out.chi2, *round_cost_initial = out.round_cost_initial, *round_cost_final = out.round_cost_final;
    double *round_lambda = out.round_lambda, *proj = out.proj;
    uint8_t *outlier = out.outlier;
    int32_t *status = out.status, *counts = out.counts, *kp_point = out.kp_point, *inliers = out.inliers, *rounds_run = out.rounds_run;
    int32_t *round_status = out.round_status, *round_iterations = out.round_iterations, *match = out.match, *dist = out.dist, *level = out.level;
    int32_t *reason = out.reason, *outcome = out.outcome, *n_cand = out.n_cand, *n_gated = out.n_gated;
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!slot || !set || !T || !T_out || n_frames < 1 || n_sets < 1) return YGZ_E_INVALID;
    if (indexed ? ((!resident && (!src.list_pt || !src.list_len)) || src.n_points < 0) : !sets) return YGZ_E_INVALID;
    if (n_frames > YGZ_SLM_MAX_FRAMES) return YGZ_E_CAPACITY;
    if (indexed ? (n_sets > YGZ_SLM_MAX_FRAMES || src.n_points > YGZ_MPA_MAX_POINTS) : n_sets > YGZ_SLM_MAX_SETS) return YGZ_E_CAPACITY;
    ygz_slm_params p;
    if (params) p = *params; else ygz_hip_default_slm_params(&p);
    if (!isfinite(p.baseline) || !isfinite(p.th) || !isfinite(p.ratio) || !isfinite(p.r_near) || !isfinite(p.r_wide) || !isfinite(p.cos_near))
        return YGZ_E_INVALID;
    if (!(p.baseline > 0) || !(p.th > 0) || !(p.ratio > 0) || !(p.r_near > 0) || !(p.r_wide > 0) || p.th_dist < 0 || p.th_dist > 256 ||
        p.min_edges < 0)
        return YGZ_E_INVALID;
    if (!ygz_pose_params_ok(p.pose)) return YGZ_E_INVALID;
    if (indexed) {
        if (src.n_points > 0 && (!src.pw || !src.desc || !src.dmax || !src.normal)) return YGZ_E_INVALID;
        if (src.stride < 1) return YGZ_E_INVALID;
    }
    for (int s = 0; s < n_sets; ++s) {
        if (src.n_pt(s) < 0 || (indexed && src.n_pt(s) > src.stride)) return YGZ_E_INVALID;
        if (!indexed && sets[s].n_pt > 0 && (!sets[s].pw || !sets[s].pt_desc || !sets[s].pt_dmax || !sets[s].pt_normal)) return YGZ_E_INVALID;
    }
    const size_t F = (size_t)n_frames;
    size_t N = 0;
    int max_pt = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (slot[f] < 0 || set[f] < 0 || set[f] >= n_sets) return YGZ_E_INVALID;
        N += (size_t)src.n_pt(set[f]);
        if (src.n_pt(set[f]) > max_pt) max_pt = src.n_pt(set[f]);
    }
    // by index: the lists some frame reads; the others are neither checked nor gathered
    std::vector<uint8_t> read_(indexed ? (size_t)n_sets : 0, 0);
    if (indexed && !resident) {
        for (int f = 0; f < n_frames; ++f) read_[(size_t)set[f]] = 1;
        for (int s = 0; s < n_sets; ++s) {
            const int32_t *row = src.list_pt + (size_t)s * (size_t)src.stride;
            for (int i = 0; read_[(size_t)s] && i < src.list_len[s]; ++i)
                if (row[i] < 0 || row[i] >= src.n_points) return YGZ_E_INVALID;
        }
    }
    if (N > YGZ_SLM_MAX_PAIRS) return YGZ_E_CAPACITY;
    if (!ygz_all_finite(T, 7 * F)) return YGZ_E_INVALID;
    if (indexed && !resident) {                                          // a resident map was checked when it went up
        const size_t n = (size_t)src.n_points;
        if (n && (!ygz_all_finite(src.pw, 3 * n) || !ygz_all_finite(src.dmax, n) || !ygz_all_finite(src.normal, 3 * n))) return YGZ_E_INVALID;
    }
    for (int s = 0; !indexed && s < n_sets; ++s) {
        const size_t n = (size_t)sets[s].n_pt;
        if (n && (!ygz_all_finite(sets[s].pw, 3 * n) || !ygz_all_finite(sets[s].pt_dmax, n) || !ygz_all_finite(sets[s].pt_normal, 3 * n))) return YGZ_E_INVALID;
    }
    if (!ctx) return YGZ_E_INVALID;
    for (int f = 0; f < n_frames; ++f)
        if (slot[f] >= ctx->prm.max_frames) return YGZ_E_INVALID;
    const int L = ctx->prm.pyramid_levels;
    if (L < 1 || L > YGZ_MAX_LEVELS) return YGZ_E_INVALID;
    if (ctx->cells > YGZ_SLOT_MAX_CELLS) return YGZ_E_CAPACITY;
    const size_t Cn = (size_t)ctx->cells, NK = F * Cn;
    if (prior)
        for (size_t f = 0; f < F; ++f) {
            const int32_t n = src.n_pt(set[f]), *row = prior + f * Cn;
            for (size_t j = 0; j < Cn; ++j)
                if (row[j] < -1 || row[j] >= n) return YGZ_E_INVALID;
        }
    for (int f = 0; f < n_frames; ++f)
        if (!ctx->pyr_valid[slot[f]]) return YGZ_E_STATE;
    if (!ctx->kp_depth || !ctx->kp_has_mp) return YGZ_E_STATE;
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }

    // the distinct slots of the call, in the order they first appear; where a frame's points begin
    std::vector<int32_t> slots, where((size_t)ctx->prm.max_frames, -1), ds(F), pt_off(F), e_off(F);
    size_t run = 0;
    for (size_t f = 0; f < F; ++f) {
        ds[f] = ygz_distinct_slot(slots, where, slot[f]);
        pt_off[f] = (int32_t)run; run += (size_t)src.n_pt(set[f]);
        e_off[f] = (int32_t)(f * Cn);
    }
    const size_t D = slots.size();

    // up: [in | the frames' tables | the sets | prior | the skip rows, zero | poses), back: [poses | the small outputs | the per-keypoint
    // outputs | the per-point outputs), then what stays on the device
    YgzBlobLayout B;
    const size_t o_in = B.add(sizeof(StIn)), o_slots = B.add_n<int32_t>(D), o_fslot = B.add_n<int32_t>(F), o_fds = B.add_n<int32_t>(F);
    const size_t o_fset = B.add_n<int32_t>(F), o_ptoff = B.add_n<int32_t>(F), o_off = B.add_n<int32_t>(F);
    const size_t o_tab = B.add_n<SlmSetTab>((size_t)n_sets);
    std::vector<SlmSetTab> tab((size_t)n_sets);
    // by index the map and the lists go up in the sets' place, and the sets' arrays lie behind everything else: k_slm_index fills them
    const size_t MP = indexed && !resident ? (size_t)src.n_points : 0, LS = indexed && !resident ? (size_t)n_sets * (size_t)src.stride : 0;
    const bool has_prior = prior || resident;
    const size_t o_mpw = B.add_n<double>(MP * 3), o_mdesc = B.add_n<uint4>(MP * 2), o_mdmax = B.add_n<double>(MP), o_mnrm = B.add_n<double>(MP * 3);
    const size_t o_lpt = B.add_n<int32_t>(LS);
    for (int s = 0; !indexed && s < n_sets; ++s) {
        const size_t n = (size_t)sets[s].n_pt;
        tab[(size_t)s].pw = B.add_n<double>(n * 3);
        tab[(size_t)s].desc = B.add_n<uint4>(n * 2);                     // 16-byte aligned: read as two uint4
        tab[(size_t)s].dmax = B.add_n<double>(n);
        tab[(size_t)s].normal = B.add_n<double>(n * 3);
        tab[(size_t)s].n_pt = sets[s].n_pt; tab[(size_t)s].pad_ = 0;
    }
    const size_t o_prior = B.add_n<int32_t>(prior ? NK : 0);
    size_t o_skip = B.add_n<uint8_t>(prior ? N : 0);
    const size_t o_pose = B.add_n<double>(F * 7), in_end = B.end;
    const size_t o_status = B.add_n<int32_t>(F), o_counts = B.add_n<int32_t>(F * 8);
    YgzPoseBlock PB;
    PB.add_results(B, F);
    size_t back_end = B.end;
    // the per-keypoint and per-point outputs, fetched up to the last one the caller asked for
    const size_t o_kpt = B.add_n<int32_t>(NK); if (kp_point) back_end = B.end;
    const size_t o_out = B.add_n<uint8_t>(NK); if (outlier) back_end = B.end;
    const size_t o_chi2 = B.add_n<double>(NK); if (chi2) back_end = B.end;
    const size_t o_match = B.add_n<int32_t>(N); if (match && N) back_end = B.end;
    const size_t o_dist = B.add_n<int32_t>(N); if (dist && N) back_end = B.end;
    const size_t o_oc = B.add_n<int32_t>(N); if (outcome && N) back_end = B.end;
    const size_t o_why = B.add_n<int32_t>(N); if (reason && N) back_end = B.end;
    const size_t o_lvl = B.add_n<int32_t>(N); if (level && N) back_end = B.end;
    const size_t o_nc = B.add_n<int32_t>(N); if (n_cand && N) back_end = B.end;
    const size_t o_ng = B.add_n<int32_t>(N); if (n_gated && N) back_end = B.end;
    const size_t o_proj = B.add_n<double>(N * 3); if (proj && N) back_end = B.end;
    const size_t o_keys = B.add_n<uint4>(N * 2);
    PB.add_edges(B, F, Cn);
    const size_t o_sets = B.add_n<StSetDev>((size_t)n_sets), o_probs = B.add_n<StProbDev>(F);
    const size_t o_gur = B.add_n<double>(D * Cn), o_taken = B.add_n<uint8_t>(has_prior ? NK : 0);
    if (resident) o_skip = B.add_n<uint8_t>(N);                          // zeroed by the hook's launches, not by the upload
    int longest = 1;
    for (int s = 0; indexed && s < n_sets; ++s) {
        const size_t n = resident ? (size_t)src.stride : read_[(size_t)s] ? (size_t)src.list_len[s] : 0;
        tab[(size_t)s].pw = B.add_n<double>(n * 3);
        tab[(size_t)s].desc = B.add_n<uint4>(n * 2);
        tab[(size_t)s].dmax = B.add_n<double>(n);
        tab[(size_t)s].normal = B.add_n<double>(n * 3);
        tab[(size_t)s].n_pt = resident ? 0 : (int32_t)n; tab[(size_t)s].pad_ = 0;   // resident: the room is n, the length comes from the hook
        if ((int)n > longest) longest = (int)n;
    }
    const size_t total = B.end;
    YgzBlob blob;
    int rc = ygz_blob_open(ctx, SCR_SLM, total, back_end, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    StIn in;
    memset(&in, 0, sizeof in);
    in.K4[0] = (double)ctx->prm.fx; in.K4[1] = (double)ctx->prm.fy; in.K4[2] = (double)ctx->prm.cx; in.K4[3] = (double)ctx->prm.cy;
    in.bf = in.K4[0] * p.baseline; in.r_near = p.r_near; in.r_wide = p.r_wide; in.cos_near = p.cos_near;
    in.w = ctx->prm.image_width; in.h = ctx->prm.image_height; in.L = L;
    memcpy(up + o_in, &in, sizeof in);
    memcpy(up + o_slots, slots.data(), D * 4); memcpy(up + o_fslot, slot, F * 4); memcpy(up + o_fds, ds.data(), F * 4);
    memcpy(up + o_fset, set, F * 4); memcpy(up + o_ptoff, pt_off.data(), F * 4); memcpy(up + o_off, e_off.data(), F * 4);
    memcpy(up + o_tab, tab.data(), (size_t)n_sets * sizeof(SlmSetTab));
    if (MP) {
        memcpy(up + o_mpw, src.pw, MP * 24); memcpy(up + o_mdesc, src.desc, MP * 32);
        memcpy(up + o_mdmax, src.dmax, MP * 8); memcpy(up + o_mnrm, src.normal, MP * 24);
    }
    if (LS) memcpy(up + o_lpt, src.list_pt, LS * 4);
    for (int s = 0; !indexed && s < n_sets; ++s) {
        const size_t n = (size_t)sets[s].n_pt;
        if (!n) continue;
        const SlmSetTab &t = tab[(size_t)s];
        memcpy(up + t.pw, sets[s].pw, n * 24); memcpy(up + t.desc, sets[s].pt_desc, n * 32);
        memcpy(up + t.dmax, sets[s].pt_dmax, n * 8); memcpy(up + t.normal, sets[s].pt_normal, n * 24);
    }
    if (prior) { memcpy(up + o_prior, prior, NK * 4); memset(up + o_skip, 0, N); }
    memcpy(up + o_pose, T, F * 56);
    if ((rc = ygz_blob_upload(ctx, blob, in_end)) != YGZ_OK) return rc;

    SlmDev A;
    memset(&A, 0, sizeof A);
    A.kp_px = ctx->kp_px; A.kp_level = ctx->kp_level; A.kp_desc = ctx->kp_desc; A.n_kp = ctx->n_kp;
    A.kp_depth = ctx->kp_depth; A.kp_has_mp = ctx->kp_has_mp;
    A.block = dev; A.set_tab = ygz_at<const SlmSetTab>(dev, o_tab);
    A.slots = ygz_at<const int32_t>(dev, o_slots); A.fr_slot = ygz_at<const int32_t>(dev, o_fslot); A.fr_dslot = ygz_at<const int32_t>(dev, o_fds);
    A.fr_set = ygz_at<const int32_t>(dev, o_fset); A.pt_off = ygz_at<const int32_t>(dev, o_ptoff);
    A.prior = prior ? ygz_at<const int32_t>(dev, o_prior) : nullptr;
    A.poses = ygz_at<double>(dev, o_pose);
    A.g_ur = ygz_at<double>(dev, o_gur); A.kp_taken = dev + o_taken; A.pt_skip = dev + o_skip;
    A.sets = ygz_at<StSetDev>(dev, o_sets); A.probs = ygz_at<StProbDev>(dev, o_probs);
    A.keys = ygz_at<uint32_t>(dev, o_keys); A.n_cand = ygz_at<int32_t>(dev, o_nc); A.n_gated = ygz_at<int32_t>(dev, o_ng);
    A.level = ygz_at<int32_t>(dev, o_lvl); A.reason = ygz_at<int32_t>(dev, o_why); A.proj = ygz_at<double>(dev, o_proj);
    A.match = ygz_at<int32_t>(dev, o_match); A.dist = ygz_at<int32_t>(dev, o_dist); A.outcome = ygz_at<int32_t>(dev, o_oc);
    A.kp_point = ygz_at<int32_t>(dev, o_kpt);
    ygz_slot_edges_bind(A.E, dev, PB, o_out, o_chi2);
    A.status = ygz_at<int32_t>(dev, o_status); A.counts = ygz_at<int32_t>(dev, o_counts);
    A.bf = in.bf; A.th = p.th; A.ratio = p.ratio;
    A.cells = ctx->cells; A.n_frames = n_frames; A.n_slots = (int)D; A.n_sets = n_sets; A.th_dist = p.th_dist; A.min_edges = p.min_edges;

    PoptArgs G;
    memset(&G, 0, sizeof G);
    ygz_popt_bind(G, dev, PB, o_off, o_pose);
    ygz_popt_set_params(G, in.K4, p.baseline, p.pose);

    int widest = ctx->cells > n_frames ? ctx->cells : n_frames;
    if (n_sets > widest) widest = n_sets;
    const unsigned bx = (unsigned)ygz_div_up(ctx->cells, SL_LANES), bt = (unsigned)ygz_div_up(widest, SL_LANES);
    const unsigned sx = (unsigned)ygz_div_up(max_pt > 0 ? max_pt : 1, ST_DEV_LANES);
    if (indexed) {
        SlmIndexDev X;
        X.block = dev; X.tab = A.set_tab;
        X.pw = ygz_at<const double>(dev, o_mpw); X.desc = ygz_at<const uint4>(dev, o_mdesc); X.dmax = ygz_at<const double>(dev, o_mdmax);
        X.normal = ygz_at<const double>(dev, o_mnrm); X.list_pt = ygz_at<const int32_t>(dev, o_lpt); X.stride = src.stride;
        if (resident) {
            SlmResidentDev R;
            R.tab = ygz_at<SlmSetTab>(dev, o_tab); R.pt_skip = dev + o_skip; R.n_frames = n_frames; R.stride = src.stride; R.cells = ctx->cells;
            R.list_pt = nullptr; R.prior = nullptr;
            if ((rc = src.resident(ctx, src.user, R)) != YGZ_OK) return rc;
            X.pw = src.pw; X.desc = reinterpret_cast<const uint4 *>(src.desc); X.dmax = src.dmax; X.normal = src.normal;
            X.list_pt = R.list_pt; A.prior = R.prior;
        }
        src.index(ctx, X, n_sets, longest);
    }
    YGZ_LAUNCH(ctx, KID_SLM_GATHER, k_slm_gather, dim3(bt, (unsigned)(D + (has_prior ? F : 0))), dim3(SL_LANES), A);
    YGZ_LAUNCH(ctx, KID_STRACK_SEARCH, k_strack_search, dim3(sx, (unsigned)n_frames), dim3(ST_DEV_LANES), ygz_at<const StIn>(dev, o_in), A.sets,
               A.probs, A.keys, A.n_cand, A.n_gated, A.level, A.reason, A.proj);
    YGZ_LAUNCH(ctx, KID_SLM_RESOLVE, k_slm_resolve, dim3((unsigned)n_frames), dim3(SL_LANES), A);
    YGZ_LAUNCH(ctx, KID_POSE_OPT, k_pose_opt, dim3((unsigned)n_frames), dim3(PT_DEV_THREADS), G);
    YGZ_LAUNCH(ctx, KID_SLM_SCATTER, k_slm_scatter, dim3(bx, (unsigned)n_frames), dim3(SL_LANES), A);
    if ((rc = ygz_blob_fetch(ctx, blob, o_pose, back_end)) != YGZ_OK) return rc;
    memcpy(T_out, up + o_pose, F * 56);
    if (status) memcpy(status, up + o_status, F * 4);
    if (counts) memcpy(counts, up + o_counts, F * 32);
    PB.copy_results(up, F, inliers, rounds_run, round_status, round_iterations, round_cost_initial, round_cost_final, round_lambda);
    if (kp_point) memcpy(kp_point, up + o_kpt, NK * 4);
    if (outlier) memcpy(outlier, up + o_out, NK);
    if (chi2) memcpy(chi2, up + o_chi2, NK * 8);
    if (N) {
        if (match) memcpy(match, up + o_match, N * 4);
        if (dist) memcpy(dist, up + o_dist, N * 4);
        if (outcome) memcpy(outcome, up + o_oc, N * 4);
        if (reason) memcpy(reason, up + o_why, N * 4);
        if (level) memcpy(level, up + o_lvl, N * 4);
        if (n_cand) memcpy(n_cand, up + o_nc, N * 4);
        if (n_gated) memcpy(n_gated, up + o_ng, N * 4);
        if (proj) memcpy(proj, up + o_proj, N * 24);
    }
    return YGZ_OK;
}
