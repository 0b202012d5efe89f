// SVO -- stereo odometry on resident slots: ORB-SLAM2's TrackWithMotionModel on the last frame's own depths, for any number of (last, current)
// slot pairs in one call.  Nothing in the reference, whose tracker is monocular.  The result is the composition of two frozen specifications,
// tests/strack_ref.c (search, claim walk, orientation rule) and tests/popt_ref.c (the u, v, uR pose optimisation), joined by three formulas
// (tests/svo_ref.py); every output is bit-identical to that composition.  k_strack_search (strack.hip) and k_pose_opt
// (popt.hip) are launched from here on tables and edges that these kernels write:
//   k_svo_gather   lane = one keypoint of one DISTINCT slot of the call: pw = (((u - cx) / fx) z, ((v - cy) / fy) z, z), the skip flag and
//                  kp_ur = u - bf / z, once per slot whether it is a pair's last frame, a pair's current frame or both.  The first lanes also write
//                  the StSetDev / StProbDev entry of every pair, n_pt and n_kp from the slots' own counts: the host reads no count.  Level,
//                  descriptor and angle are read where the extractor left them (the angle's conversion to double is exact, so it is made on use).
//   k_svo_resolve  one workgroup per pair, built for throughput over pairs.  The claim walk is a serial chain through the `taken` flags: they
//                  are a bitmap in LDS, the lists of 256 points at a time are staged in LDS by all lanes, and lane 0 walks them.  The rest is
//                  parallel: the outcome of every point from the entry the walk picked, the (float) rotation arithmetic, the 30-bin histogram in
//                  integer LDS counters, the removal, the counts, and the order-preserving compaction of the matched points into edges (ballot and
//                  popcount per wavefront, a running base).  Lane 0 decides the retry and writes the pair's entry for the second pass: th doubled,
//                  or an empty set, for which k_strack_search's blocks return at once.  Search and resolve are launched twice unconditionally.
//   k_svo_scatter  outlier and chi2 of the edges back to point order.
// FP64 in the stated order; integer atomics on LDS counters only; no floating-point atomic, no wait for another workgroup, no scratch, no
// environment switch; every loop is bounded by a count known at entry; every index read from a key is checked against n_kp before it addresses
// memory.  One packed upload, the launches, one copy back, one wait.
#include "ygz_internal.h"
#include "strack_dev.h"
#include "popt_dev.h"
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)
#include "ur_dev.h"                     // the right column of a resident keypoint: slm.hip and srk.hip gather the same way
#include "slot_pose_dev.h"              // the edges of k_pose_opt and the rotation rule: slm.hip and srk.hip compact and scatter the same way

#define SV_LANES      256

struct SvoDev {
    // the resident keypoints [max_frames][cells]
    const double *kp_px; const int32_t *kp_level; const float *kp_angle; const uint32_t *kp_desc; const int32_t *n_kp;
    const double *kp_depth; const uint8_t *kp_has_mp;
    // the call: distinct slots, per pair the indices of its two slots in that list, the slots themselves, direction and entry pose
    const int32_t *slots, *pair_dl, *pair_dc, *pair_l, *pair_c, *direction;
    double *poses;                                   // [n_pairs][7]: T_init in, T_rel out (k_pose_opt)
    // per distinct slot [n_slots][cells]
    double *g_pw, *g_ur; uint8_t *g_skip;
    StSetDev *sets;                                  // [n_pairs + 1]: the last one is empty
    StProbDev *probs1, *probs2;                      // [n_pairs]: the first pass, the retry
    // per (pair, point) [n_pairs][cells]
    uint32_t *keys; int32_t *n_cand, *n_gated, *level, *reason; double *proj;
    int32_t *match, *dist, *outcome;
    SlotEdges E;                                     // the edges of pair p: [p * cells, edge_end[p])
    int32_t *retry, *status, *counts, *rot;
    double K4[4], bf, th;
    int cells, n_pairs, n_slots, th_dist, check_orientation, min_matches;
};

__global__ __launch_bounds__(SV_LANES) void k_svo_gather(SvoDev A)
{
    const int d = blockIdx.y, i = blockIdx.x * SV_LANES + threadIdx.x;
    const int s = A.slots[d];
    if (i < ygz_slot_count(A.n_kp, s, A.cells)) {
        const size_t g = (size_t)s * A.cells + i, o = (size_t)d * A.cells + i;
        const double u = A.kp_px[2 * g], v = A.kp_px[2 * g + 1], z = A.kp_depth[g];
        const bool has = ygz_kp_has_depth(A.kp_has_mp[g], z);          // a NaN depth compares false
        double x = 0, y = 0, zz = 0, ur = -1.0;
        if (has) {
            x = ((u - A.K4[2]) / A.K4[0]) * z;
            y = ((v - A.K4[3]) / A.K4[1]) * z;
            zz = z;
            ur = ygz_kp_right_column(u, z, A.bf);
        }
        A.g_pw[3 * o] = x; A.g_pw[3 * o + 1] = y; A.g_pw[3 * o + 2] = zz;
        A.g_ur[o] = ur;
        A.g_skip[o] = has ? 0 : 1;
    }
    if (d != 0) return;
    if (i < A.n_pairs) {
        const int L = A.pair_l[i], C = A.pair_c[i];
        const size_t oL = (size_t)L * A.cells, oC = (size_t)C * A.cells, gL = (size_t)A.pair_dl[i] * A.cells, gC = (size_t)A.pair_dc[i] * A.cells;
        StSetDev S;
        S.pw = A.g_pw + 3 * gL; S.pt_desc = A.kp_desc + 8 * oL; S.pt_level = A.kp_level + oL; S.pt_dmax = nullptr; S.pt_normal = nullptr;
        S.n_pt = ygz_slot_count(A.n_kp, L, A.cells); S.pad_ = 0;
        A.sets[i] = S;
        StProbDev P;
        P.kp_px = A.kp_px + 2 * oC; P.kp_level = A.kp_level + oC; P.kp_desc = A.kp_desc + 8 * oC; P.kp_ur = A.g_ur + gC; P.kp_taken = nullptr;
        P.pt_skip = A.g_skip + gL;
        P.n_kp = ygz_slot_count(A.n_kp, C, A.cells); P.set = i; P.pt_off = i * A.cells; P.mode = 0; P.direction = A.direction[i]; P.pad_ = 0;
        P.th = A.th;
#pragma unroll
        for (int k = 0; k < 7; ++k) P.T[k] = A.poses[7 * (size_t)i + k];
        A.probs1[i] = P;
    }
    if (i == 0) {
        StSetDev S;
        S.pw = nullptr; S.pt_desc = nullptr; S.pt_level = nullptr; S.pt_dmax = nullptr; S.pt_normal = nullptr; S.n_pt = 0; S.pad_ = 0;
        A.sets[A.n_pairs] = S;
    }
}

enum { SV_N_DEPTH = 0, SV_N_SEARCHED, SV_N_OVER, SV_N_ROT, SV_N_CLAIMED, SV_N_COUNTERS };

__global__ __launch_bounds__(SV_LANES) void k_svo_resolve(SvoDev A, int pass)
{
    __shared__ uint32_t s_taken[YGZ_SLOT_MAX_CELLS / 32];
    __shared__ uint4 s_key[SV_LANES][2];
    __shared__ uint32_t s_pick[SV_LANES];
    __shared__ int s_hist[30], s_ind[3], s_cnt[SV_N_COUNTERS], s_wave[SV_LANES / 64];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (pass == 1 && !A.retry[p]) return;                                // the same in every lane: the first pass stands
    const StProbDev &P = (pass ? A.probs2 : A.probs1)[p];
    const int cells = A.cells, n_pt = A.sets[p].n_pt, n_kp = P.n_kp;
    const size_t base = (size_t)p * cells;
    const uint32_t idx_mask = (1u << ST_DEV_IDX_BITS) - 1;
    const size_t oL = (size_t)A.pair_l[p] * cells, oC = (size_t)A.pair_c[p] * cells;

    for (int w = tid; w < (n_kp + 31) / 32; w += SV_LANES) s_taken[w] = 0;
    if (tid < 30) s_hist[tid] = 0;
    if (tid < SV_N_COUNTERS) s_cnt[tid] = 0;
    if (tid < 3) s_ind[tid] = -1;
    // past the last keypoint: -1 (proj 0); the points with a depth
    int c_depth = 0;
    for (int i = tid; i < cells; i += SV_LANES) {
        const size_t g = base + i;
        if (i < n_pt) { c_depth += P.pt_skip[i] ? 0 : 1; continue; }
        A.match[g] = -1; A.dist[g] = -1; A.outcome[g] = -1; A.level[g] = -1; A.reason[g] = -1; A.n_cand[g] = -1; A.n_gated[g] = -1;
        A.proj[3 * g] = 0; A.proj[3 * g + 1] = 0; A.proj[3 * g + 2] = 0;
    }
    __syncthreads();

    // ---- step 8: the claim walk.  A point's list is sorted and padded with empty entries, and a point that was not searched has an empty list:
    // the first entry whose keypoint is free is e1, whatever n_cand and the reason say
    int c_search = 0, c_over = 0, c_claim = 0, c_rot = 0;
    for (int c0 = 0; c0 < n_pt; c0 += SV_LANES) {
        const int i = c0 + tid;
        if (i < n_pt) {
            const uint4 *k = reinterpret_cast<const uint4 *>(A.keys + YGZ_STRACK_TOPK * (base + i));
            s_key[tid][0] = k[0]; s_key[tid][1] = k[1];
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = min(SV_LANES, n_pt - c0);
            for (int t = 0; t < cnt; ++t) {
                const uint4 a = s_key[t][0], b = s_key[t][1];
                uint32_t pick = ST_DEV_NO_KEY;
                // the reads of the bitmap are independent; the earliest free entry wins, so the last one is tried first
#define SV_TRY_(key) { const uint32_t k_ = (key), j_ = k_ & idx_mask;                                                  \
                       const bool in_ = k_ != ST_DEV_NO_KEY && j_ < (uint32_t)n_kp;                                     \
                       const uint32_t word_ = s_taken[in_ ? (j_ >> 5) : 0];                                             \
                       if (in_ && !((word_ >> (j_ & 31)) & 1u)) pick = k_; }
                SV_TRY_(b.w) SV_TRY_(b.z) SV_TRY_(b.y) SV_TRY_(b.x) SV_TRY_(a.w) SV_TRY_(a.z) SV_TRY_(a.y) SV_TRY_(a.x)
#undef SV_TRY_
                if (pick != ST_DEV_NO_KEY && (int)(pick >> ST_DEV_IDX_BITS) <= A.th_dist) s_taken[(pick & idx_mask) >> 5] |= 1u << (pick & 31);
                s_pick[t] = pick;
            }
        }
        __syncthreads();
        if (i < n_pt) {
            const size_t g = base + i;
            int m = -1, d = -1, oc = -1;
            if (A.reason[g] == 0) {
                ++c_search;
                if (A.n_cand[g] > YGZ_STRACK_TOPK) ++c_over;
                const uint32_t pick = s_pick[tid];
                const int d1 = (int)(pick >> ST_DEV_IDX_BITS);
                if (pick == ST_DEV_NO_KEY) oc = 1;
                else if (d1 > A.th_dist) oc = 2;
                else { oc = 0; m = (int)(pick & idx_mask); d = d1; ++c_claim; }
            }
            A.match[g] = m; A.dist[g] = d; A.outcome[g] = oc;             // read again below by the lane that wrote them
        }
    }

    // ---- step 9: the rotation histogram, its three maxima, the removal
    if (A.check_orientation) {
        for (int i = tid; i < n_pt; i += SV_LANES) {
            const int m = A.match[base + i];
            if (m < 0 || m >= n_kp) continue;
            const int bin = ygz_rot_bin(A.kp_angle[oL + i], A.kp_angle[oC + m]);
            if (bin >= 0) atomicAdd(&s_hist[bin], 1);
        }
        __syncthreads();
        if (tid == 0) ygz_rot_top3(s_hist, s_ind);
        __syncthreads();
        const int i0 = s_ind[0], i1 = s_ind[1], i2 = s_ind[2];
        for (int i = tid; i < n_pt; i += SV_LANES) {
            const size_t g = base + i;
            const int m = A.match[g];
            if (m < 0 || m >= n_kp) continue;
            const int bin = ygz_rot_bin(A.kp_angle[oL + i], A.kp_angle[oC + m]);
            if (bin >= 0 && (bin == i0 || bin == i1 || bin == i2)) continue;
            A.match[g] = -1; A.dist[g] = -1; A.outcome[g] = 4; ++c_rot;     // the keypoint stays claimed
        }
    }
    if (c_depth) atomicAdd(&s_cnt[SV_N_DEPTH], c_depth);
    if (c_search) atomicAdd(&s_cnt[SV_N_SEARCHED], c_search);
    if (c_over) atomicAdd(&s_cnt[SV_N_OVER], c_over);
    if (c_claim) atomicAdd(&s_cnt[SV_N_CLAIMED], c_claim);
    if (c_rot) atomicAdd(&s_cnt[SV_N_ROT], c_rot);
    __syncthreads();
    const int n_match = s_cnt[SV_N_CLAIMED] - s_cnt[SV_N_ROT];
    const bool again = pass == 0 && n_match < A.min_matches;             // the same in every lane
    const int status = n_match < A.min_matches ? 1 : 0;
    if (tid == 0) {
        int32_t *c = A.counts + 8 * (size_t)p;
        c[0] = n_pt; c[1] = s_cnt[SV_N_DEPTH]; c[2] = n_kp; c[3] = n_match; c[4] = s_cnt[SV_N_SEARCHED]; c[5] = s_cnt[SV_N_OVER];
        c[6] = s_cnt[SV_N_ROT]; c[7] = pass;
        A.status[p] = status;
        if (pass == 0) {
            A.retry[p] = again ? 1 : 0;
            StProbDev &Q = A.probs2[p];                                  // the first pass's entry, with th doubled or pointed at the empty set
            Q.kp_px = P.kp_px; Q.kp_level = P.kp_level; Q.kp_desc = P.kp_desc; Q.kp_ur = P.kp_ur; Q.kp_taken = nullptr; Q.pt_skip = P.pt_skip;
            Q.n_kp = n_kp; Q.set = again ? p : A.n_pairs; Q.pt_off = P.pt_off; Q.mode = 0; Q.direction = P.direction; Q.pad_ = 0;
            Q.th = again ? P.th * 2.0 : P.th;
            for (int k = 0; k < 7; ++k) Q.T[k] = P.T[k];
        }
    }
    if (tid < 33) A.rot[33 * (size_t)p + tid] = tid < 30 ? s_hist[tid] : s_ind[tid - 30];

    // ---- the edges: the matched points in point order (none for a pair that retries or has failed)
    const bool edges = !again && status == 0;
    int running = 0;
    for (int c0 = 0; c0 < cells; c0 += SV_LANES) {
        const int i = c0 + tid;
        const int m = (edges && i < n_pt) ? A.match[base + i] : -1;
        const bool has = m >= 0 && m < n_kp;
        const int e = ygz_edge_slot<SV_LANES>(has, running, s_wave);
        if (has) {
            ygz_edge_write(A.E, base + e, A.sets[p].pw + 3 * (size_t)i, P.kp_px + 2 * (size_t)m, P.kp_ur[m], P.kp_level[m]);
            A.E.edge_of[base + i] = e;
        } else if (i < cells) A.E.edge_of[base + i] = -1;
        __syncthreads();
    }
    if (tid == 0) A.E.edge_end[p] = (int32_t)base + running;
}

__global__ __launch_bounds__(SV_LANES) void k_svo_scatter(SvoDev A)
{
    const int p = blockIdx.y, i = blockIdx.x * SV_LANES + threadIdx.x;
    if (i >= A.cells) return;
    const size_t base = (size_t)p * A.cells;
    ygz_edge_scatter(A.E, base, base + i, A.cells);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// StereoTracker's motion direction for the last camera at the identity: t_lc = -R_c^T t_c, +1 when its z is above the baseline, -1 below minus it
static int svo_direction(const double *T, double baseline)
{
    const double x = T[0], y = T[1], z = T[2], w = T[3];
    const double r02 = 2.0 * (x * z + w * y), r12 = 2.0 * (y * z - w * x), r22 = 1.0 - 2.0 * (x * x + y * y);
    const double t = -((r02 * T[4] + r12 * T[5]) + r22 * T[6]);
    return t > baseline ? 1 : (-t > baseline ? -1 : 0);
}

extern "C" {

void ygz_hip_default_svo_params(ygz_svo_params *p)
{
    if (!p) return;
    p->baseline = 0.1; p->th = 7.0; p->th_dist = 100; p->check_orientation = 1; p->min_matches = 20; p->pad = 0;
    ygz_hip_default_pose_opt_params(&p->pose);
    p->pose.baseline = p->baseline;
}

int ygz_hip_stereo_odometry_slots(ygz_hip_ctx *ctx, int n_pairs, const int32_t *last_slot, const int32_t *cur_slot, const double *T_init,
                                  const int32_t *direction, const ygz_svo_params *params, double *T_rel, int32_t *status, int32_t *counts,
                                  int32_t *match, int32_t *dist, int32_t *level, int32_t *reason, int32_t *outcome, int32_t *n_cand,
                                  int32_t *n_gated, double *proj, int32_t *rot, uint8_t *outlier, double *chi2, int32_t *inliers,
                                  int32_t *rounds_run, int32_t *round_status, int32_t *round_iterations, double *round_cost_initial,
                                  double *round_cost_final, double *round_lambda)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!last_slot || !cur_slot || !T_rel || n_pairs < 1) return YGZ_E_INVALID;
    if (n_pairs > YGZ_SVO_MAX_PAIRS) return YGZ_E_CAPACITY;
    ygz_svo_params p;
    if (params) p = *params; else ygz_hip_default_svo_params(&p);
    if (!isfinite(p.baseline) || !isfinite(p.th) || !(p.baseline > 0) || !(p.th > 0) || p.th_dist < 0 || p.th_dist > 256 || p.min_matches < 0)
        return YGZ_E_INVALID;
    if (!ygz_pose_params_ok(p.pose)) return YGZ_E_INVALID;
    const size_t Q = (size_t)n_pairs;
    if (T_init && !ygz_all_finite(T_init, 7 * Q)) return YGZ_E_INVALID;
    for (int k = 0; k < n_pairs; ++k) {
        if (direction && (direction[k] < -1 || direction[k] > 1)) return YGZ_E_INVALID;
        if (last_slot[k] < 0 || cur_slot[k] < 0 || last_slot[k] == cur_slot[k]) return YGZ_E_INVALID;
    }
    if (!ctx) return YGZ_E_INVALID;
    for (int k = 0; k < n_pairs; ++k)
        if (last_slot[k] >= ctx->prm.max_frames || cur_slot[k] >= ctx->prm.max_frames) return YGZ_E_INVALID;
    const int L = ctx->prm.pyramid_levels;
    if (L < 1 || L > YGZ_MAX_LEVELS) return YGZ_E_INVALID;
    if (ctx->cells > YGZ_SLOT_MAX_CELLS) return YGZ_E_CAPACITY;
    for (int k = 0; k < n_pairs; ++k)
        if (!ctx->pyr_valid[last_slot[k]] || !ctx->pyr_valid[cur_slot[k]]) return YGZ_E_STATE;
    if (!ctx->kp_depth || !ctx->kp_has_mp) return YGZ_E_STATE;
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }

    // the distinct slots of the call, in the order they first appear
    std::vector<int32_t> slots, where((size_t)ctx->prm.max_frames, -1), dl(Q), dc(Q), dir(Q);
    for (int k = 0; k < n_pairs; ++k) {
        dl[(size_t)k] = ygz_distinct_slot(slots, where, last_slot[k]);
        dc[(size_t)k] = ygz_distinct_slot(slots, where, cur_slot[k]);
    }
    const size_t D = slots.size(), Cn = (size_t)ctx->cells, N = Q * Cn;

    // up: [in | slots | the pairs' tables | poses), back: [poses | the small outputs | the per-point outputs), then what stays on the device
    YgzBlobLayout B;
    const size_t o_in = B.add(sizeof(StIn)), o_slots = B.add_n<int32_t>(D), o_dl = B.add_n<int32_t>(Q), o_dc = B.add_n<int32_t>(Q);
    const size_t o_pl = B.add_n<int32_t>(Q), o_pc = B.add_n<int32_t>(Q), o_dir = B.add_n<int32_t>(Q), o_off = B.add_n<int32_t>(Q);
    const size_t o_pose = B.add_n<double>(Q * 7), in_end = B.end;
    const size_t o_status = B.add_n<int32_t>(Q), o_counts = B.add_n<int32_t>(Q * 8), o_rot = B.add_n<int32_t>(Q * 33);
    YgzPoseBlock PB;
    PB.add_results(B, Q);
    size_t back_end = B.end;
    // the per-point outputs, fetched up to the last one the caller asked for
    const size_t o_match = B.add_n<int32_t>(N); if (match) back_end = B.end;
    const size_t o_out = B.add_n<uint8_t>(N); if (outlier) back_end = B.end;
    const size_t o_chi2 = B.add_n<double>(N); if (chi2) back_end = B.end;
    const size_t o_dist = B.add_n<int32_t>(N); if (dist) back_end = B.end;
    const size_t o_oc = B.add_n<int32_t>(N); if (outcome) back_end = B.end;
    const size_t o_why = B.add_n<int32_t>(N); if (reason) back_end = B.end;
    const size_t o_lvl = B.add_n<int32_t>(N); if (level) back_end = B.end;
    const size_t o_nc = B.add_n<int32_t>(N); if (n_cand) back_end = B.end;
    const size_t o_ng = B.add_n<int32_t>(N); if (n_gated) back_end = B.end;
    const size_t o_proj = B.add_n<double>(N * 3); if (proj) back_end = B.end;
    const size_t o_keys = B.add_n<uint4>(N * 2);
    PB.add_edges(B, Q, Cn);
    const size_t o_retry = B.add_n<int32_t>(Q);
    const size_t o_sets = B.add_n<StSetDev>(Q + 1), o_p1 = B.add_n<StProbDev>(Q), o_p2 = B.add_n<StProbDev>(Q);
    const size_t o_gpw = B.add_n<double>(D * Cn * 3), o_gur = B.add_n<double>(D * Cn), o_gskip = B.add_n<uint8_t>(D * Cn), total = B.end;
    YgzBlob blob;
    int rc = ygz_blob_open(ctx, SCR_SVO, total, back_end, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    StIn in;
    memset(&in, 0, sizeof in);
    in.K4[0] = (double)ctx->prm.fx; in.K4[1] = (double)ctx->prm.fy; in.K4[2] = (double)ctx->prm.cx; in.K4[3] = (double)ctx->prm.cy;
    in.bf = in.K4[0] * p.baseline;
    in.w = ctx->prm.image_width; in.h = ctx->prm.image_height; in.L = L;
    memcpy(up + o_in, &in, sizeof in);
    memcpy(up + o_slots, slots.data(), D * 4); memcpy(up + o_dl, dl.data(), Q * 4); memcpy(up + o_dc, dc.data(), Q * 4);
    memcpy(up + o_pl, last_slot, Q * 4); memcpy(up + o_pc, cur_slot, Q * 4);
    double *pose0 = ygz_at<double>(up, o_pose);
    int32_t *off = ygz_at<int32_t>(up, o_off);
    for (size_t k = 0; k < Q; ++k) {
        for (int e = 0; e < 7; ++e) pose0[7 * k + e] = T_init ? T_init[7 * k + e] : (e == 3 ? 1.0 : 0.0);
        dir[k] = direction ? direction[k] : svo_direction(pose0 + 7 * k, p.baseline);
        off[k] = (int32_t)(k * Cn);
    }
    memcpy(up + o_dir, dir.data(), Q * 4);
    if ((rc = ygz_blob_upload(ctx, blob, in_end)) != YGZ_OK) return rc;

    SvoDev A;
    memset(&A, 0, sizeof A);
    A.kp_px = ctx->kp_px; A.kp_level = ctx->kp_level; A.kp_angle = ctx->kp_angle; A.kp_desc = ctx->kp_desc; A.n_kp = ctx->n_kp;
    A.kp_depth = ctx->kp_depth; A.kp_has_mp = ctx->kp_has_mp;
    A.slots = ygz_at<const int32_t>(dev, o_slots); A.pair_dl = ygz_at<const int32_t>(dev, o_dl); A.pair_dc = ygz_at<const int32_t>(dev, o_dc);
    A.pair_l = ygz_at<const int32_t>(dev, o_pl); A.pair_c = ygz_at<const int32_t>(dev, o_pc); A.direction = ygz_at<const int32_t>(dev, o_dir);
    A.poses = ygz_at<double>(dev, o_pose);
    A.g_pw = ygz_at<double>(dev, o_gpw); A.g_ur = ygz_at<double>(dev, o_gur); A.g_skip = dev + o_gskip;
    A.sets = ygz_at<StSetDev>(dev, o_sets); A.probs1 = ygz_at<StProbDev>(dev, o_p1); A.probs2 = ygz_at<StProbDev>(dev, o_p2);
    A.keys = ygz_at<uint32_t>(dev, o_keys); A.n_cand = ygz_at<int32_t>(dev, o_nc); A.n_gated = ygz_at<int32_t>(dev, o_ng);
    A.level = ygz_at<int32_t>(dev, o_lvl); A.reason = ygz_at<int32_t>(dev, o_why); A.proj = ygz_at<double>(dev, o_proj);
    A.match = ygz_at<int32_t>(dev, o_match); A.dist = ygz_at<int32_t>(dev, o_dist); A.outcome = ygz_at<int32_t>(dev, o_oc);
    ygz_slot_edges_bind(A.E, dev, PB, o_out, o_chi2);
    A.retry = ygz_at<int32_t>(dev, o_retry); A.status = ygz_at<int32_t>(dev, o_status);
    A.counts = ygz_at<int32_t>(dev, o_counts); A.rot = ygz_at<int32_t>(dev, o_rot);
    for (int k = 0; k < 4; ++k) A.K4[k] = in.K4[k];
    A.bf = in.bf; A.th = p.th;
    A.cells = ctx->cells; A.n_pairs = n_pairs; A.n_slots = (int)D; A.th_dist = p.th_dist; A.check_orientation = p.check_orientation;
    A.min_matches = p.min_matches;

    PoptArgs G;
    memset(&G, 0, sizeof G);
    ygz_popt_bind(G, dev, PB, o_off, o_pose);
    ygz_popt_set_params(G, in.K4, p.baseline, p.pose);

    const unsigned bx = (unsigned)ygz_div_up(ctx->cells, SV_LANES), bt = (unsigned)ygz_div_up(ctx->cells > n_pairs ? ctx->cells : n_pairs, SV_LANES);
    const dim3 search_grid((unsigned)ygz_div_up(ctx->cells, ST_DEV_LANES), (unsigned)n_pairs);
    YGZ_LAUNCH(ctx, KID_SVO_GATHER, k_svo_gather, dim3(bt, (unsigned)D), dim3(SV_LANES), A);
    for (int pass = 0; pass < 2; ++pass) {                               // the retry is decided on the device: both passes are always launched
        YGZ_LAUNCH(ctx, KID_STRACK_SEARCH, k_strack_search, search_grid, dim3(ST_DEV_LANES), ygz_at<const StIn>(dev, o_in), A.sets,
                   pass ? A.probs2 : A.probs1, A.keys, A.n_cand, A.n_gated, A.level, A.reason, A.proj);
        YGZ_LAUNCH(ctx, KID_SVO_RESOLVE, k_svo_resolve, dim3((unsigned)n_pairs), dim3(SV_LANES), A, pass);
    }
    YGZ_LAUNCH(ctx, KID_POSE_OPT, k_pose_opt, dim3((unsigned)n_pairs), dim3(PT_DEV_THREADS), G);
    YGZ_LAUNCH(ctx, KID_SVO_SCATTER, k_svo_scatter, dim3(bx, (unsigned)n_pairs), dim3(SV_LANES), A);
    if ((rc = ygz_blob_fetch(ctx, blob, o_pose, back_end)) != YGZ_OK) return rc;
    memcpy(T_rel, up + o_pose, Q * 56);
    if (status) memcpy(status, up + o_status, Q * 4);
    if (counts) memcpy(counts, up + o_counts, Q * 32);
    if (rot) memcpy(rot, up + o_rot, Q * 132);
    PB.copy_results(up, Q, inliers, rounds_run, round_status, round_iterations, round_cost_initial, round_cost_final, round_lambda);
    if (match) memcpy(match, up + o_match, N * 4);
    if (outlier) memcpy(outlier, up + o_out, N);
    if (chi2) memcpy(chi2, up + o_chi2, N * 8);
    if (dist) memcpy(dist, up + o_dist, N * 4);
    if (outcome) memcpy(outcome, up + o_oc, N * 4);
    if (reason) memcpy(reason, up + o_why, N * 4);
    if (level) memcpy(level, up + o_lvl, N * 4);
    if (n_cand) memcpy(n_cand, up + o_nc, N * 4);
    if (n_gated) memcpy(n_gated, up + o_ng, N * 4);
    if (proj) memcpy(proj, up + o_proj, N * 24);
    return YGZ_OK;
}

}  // extern "C"
