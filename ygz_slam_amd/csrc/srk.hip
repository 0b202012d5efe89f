// SRK -- stereo reference-keyframe tracking on resident slots: ORB-SLAM2's TrackReferenceKeyFrame (SearchByBoW between the reference keyframe
// and the frame, then the u, v, uR pose optimisation on the associations) for any number of resident frames in one call.  Nothing in the
// reference, whose tracker is monocular.  The result is the composition of frozen specifications, yo_search_by_bow and yo_bow_orientation of
// oracle/bow.c and tests/popt_ref.c, joined by the formulas of DESIGN.md section 29 (tests/srk_ref.py); every output is bit-identical to that
// composition.  k_bow_transform, k_bow_match<0> (bow.hip) and k_pose_opt (popt.hip) are launched from here on tables and edges that these
// kernels write:
//   k_srk_gather   pass 0, rows 0 .. n_slots - 1: lane = one keypoint of one DISTINCT slot of the call, kp_ur = u - bf / z once per slot; the
//                  first lanes of row 0 also write the count row k_bow_transform reads (a slot's own count, clamped to the cell count, 0 for a
//                  slot the call does not name) and every frame's BowPair: the host reads no count.  Pass 1, behind k_bow_transform, rows 0 ..
//                  n_keyframes - 1: lane = one keypoint of one keyframe, the node row with -1 where the keypoint carries no point.
//   k_srk_resolve  one workgroup per frame.  The claim is the smallest i per frame keypoint j: an integer atomicMin on the frame's int32 row
//                  of the packed block, whose result does not depend on the order.  The rotation histogram of the claimed matches in integer
//                  LDS counters, one lane takes the three maxima; then outcomes, counts, the point every frame keypoint ends with, and the
//                  order-preserving compaction of the edges over KEYPOINTS (ballot and popcount with a running base), pw fetched from the set.
//   k_srk_scatter  outlier and chi2 of the edges back to keypoint order, prior = kp_point without the outliers, status 2.
// FP64 in the stated order; integer atomics only; no floating-point atomic, no wait for another workgroup, no scratch, no environment switch;
// every loop is a `for` over a count known at entry; every index read from kf_point or from a match is checked against n_pt / n_kp before it
// addresses memory.  One packed upload, seven launches, one copy back, one wait.
#include "ygz_internal.h"
#include "bow_dev.h"
#include "popt_dev.h"
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)
#include "ur_dev.h"
#include "slot_pose_dev.h"

#define SR_LANES      256
#define SR_FREE       0x7fffffff         // a frame keypoint that no keyframe feature names

struct SrkSetTab { uint64_t pw; int32_t n_pt, pad_; };                  // byte offset of a set's points in the packed block

struct SrkDev {
    // the resident keypoints [max_frames][cells]
    const double *kp_px; const int32_t *kp_level; const uint32_t *kp_desc; const float *kp_angle; const int32_t *n_kp; const double *kp_depth;
    const uint8_t *kp_has_mp; const int32_t *kp_node;
    // the call: the packed block, the sets' table, the distinct slots, which slots of [slot_min, slot_min + span) the call names, the
    // keyframes (slot, set, the point behind every keypoint [n_kf][cells]), per frame its slot, that slot's place in the list, its keyframe
    const uint8_t *block; const SrkSetTab *set_tab;
    const int32_t *slots, *named, *kf_slot, *kf_set, *kf_point, *fr_slot, *fr_dslot, *fr_kf;
    double *g_ur;                                    // [n_slots][cells]
    int32_t *bow_n;                                  // [span]: what k_bow_transform takes for the slots' counts
    int32_t *node1;                                  // [n_kf][cells]: the keyframe's FeatureVector nodes, -1 without a point
    BowPair *pairs; int32_t *bow_cnt;                // [n_frames]
    // per (frame, keyframe keypoint) [n_frames][cells]
    int32_t *match12, *outcome;
    // per (frame, frame keypoint) [n_frames][cells]
    int32_t *holder, *kp_point, *prior;
    SlotEdges E;                                     // the edges of frame f: [f * cells, edge_end[f])
    int32_t *status, *counts, *rot; const int32_t *inliers;
    double bf;
    int cells, n_frames, n_slots, n_kf, slot_min, span, check_orientation, min_matches, min_inliers;
};

__global__ __launch_bounds__(SR_LANES) void k_srk_gather(SrkDev A, int pass)
{
    const int y = blockIdx.y, i = blockIdx.x * SR_LANES + threadIdx.x;
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
    if (i < A.n_frames) {
        const int k = A.fr_kf[i], s1 = A.kf_slot[k], s2 = A.fr_slot[i];
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

enum { SR_N_UR = 0, SR_N_POINT, SR_N_MATCH, SR_N_LOST, SR_N_ROT, SR_N_COUNTERS };

__global__ __launch_bounds__(SR_LANES) void k_srk_resolve(SrkDev A)
{
    __shared__ int s_hist[30], s_ind[3], s_cnt[SR_N_COUNTERS], s_wave[SR_LANES / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int k = A.fr_kf[f], s1 = A.kf_slot[k], s2 = A.fr_slot[f];
    const int cells = A.cells, n1 = ygz_slot_count(A.n_kp, s1, A.cells), n2 = ygz_slot_count(A.n_kp, s2, A.cells);
    const SrkSetTab S = A.set_tab[A.kf_set[k]];
    const int n_pt = S.n_pt;
    const double *pw = reinterpret_cast<const double *>(A.block + S.pw);
    const size_t kb = (size_t)f * cells, o1 = (size_t)s1 * cells, o2 = (size_t)s2 * cells;
    const int32_t *kfp = A.kf_point + (size_t)k * cells;
    const double *ur = A.g_ur + (size_t)A.fr_dslot[f] * cells;
    int32_t *m12 = A.match12 + kb, *holder = A.holder + kb;

    if (tid < 30) s_hist[tid] = 0;
    if (tid < 3) s_ind[tid] = -1;
    if (tid < SR_N_COUNTERS) s_cnt[tid] = 0;
    // ---- every frame keypoint is free; those with a right column
    int c_ur = 0;
    for (int j0 = 0; j0 < cells; j0 += SR_LANES) {
        const int j = j0 + tid;
        if (j < cells) holder[j] = SR_FREE;
        if (j < n2) c_ur += ur[j] >= 0 ? 1 : 0;
    }
    __syncthreads();

    // ---- step 4, the claim: frame keypoint j goes to the smallest i that names it (k_bow_match wrote m12[i] for every i < n1)
    int c_pt = 0, c_match = 0;
    for (int i0 = 0; i0 < n1; i0 += SR_LANES) {
        const int i = i0 + tid;
        if (i >= n1) continue;
        const bool has = kfp[i] >= 0;
        const int m = m12[i];
        c_pt += has ? 1 : 0;
        if (has && m >= 0 && m < n2) { ++c_match; atomicMin(&holder[m], i); }
    }
    __syncthreads();

    // ---- step 5: the rotation histogram of the claimed matches and its three maxima
    if (A.check_orientation) {
        for (int i0 = 0; i0 < n1; i0 += SR_LANES) {
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
    for (int i0 = 0; i0 < cells; i0 += SR_LANES) {
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
    if (c_ur) atomicAdd(&s_cnt[SR_N_UR], c_ur);
    if (c_pt) atomicAdd(&s_cnt[SR_N_POINT], c_pt);
    if (c_match) atomicAdd(&s_cnt[SR_N_MATCH], c_match);
    if (c_lost) atomicAdd(&s_cnt[SR_N_LOST], c_lost);
    if (c_rot) atomicAdd(&s_cnt[SR_N_ROT], c_rot);
    __syncthreads();                                                     // the counters, and the outcomes as their lanes left them
    const int n_edges = s_cnt[SR_N_MATCH] - s_cnt[SR_N_LOST] - s_cnt[SR_N_ROT];
    const int status = n_edges < A.min_matches ? 1 : 0;                  // the same in every lane
    if (tid == 0) {
        int32_t *c = A.counts + 8 * (size_t)f;
        c[0] = n1; c[1] = s_cnt[SR_N_POINT]; c[2] = n2; c[3] = s_cnt[SR_N_UR]; c[4] = s_cnt[SR_N_MATCH]; c[5] = s_cnt[SR_N_LOST];
        c[6] = s_cnt[SR_N_ROT]; c[7] = n_edges;
        A.status[f] = status;
    }
    if (tid < 33) A.rot[33 * (size_t)f + tid] = tid < 30 ? s_hist[tid] : s_ind[tid - 30];

    // ---- the point behind every frame keypoint, and the edges in keypoint order (none for a frame with too few)
    int running = 0;
    for (int j0 = 0; j0 < cells; j0 += SR_LANES) {
        const int j = j0 + tid;
        int p = -1;
        if (j < n2) {
            const int i = holder[j];
            if (i >= 0 && i < n1 && A.outcome[kb + i] == 0) p = kfp[i];
        }
        if (j < cells) A.kp_point[kb + j] = p;
        const bool has = status == 0 && p >= 0 && p < n_pt;
        const int e = ygz_edge_slot<SR_LANES>(has, running, s_wave);
        if (has) {
            ygz_edge_write(A.E, kb + e, pw + 3 * (size_t)p, A.kp_px + 2 * (o2 + j), ur[j], A.kp_level[o2 + j]);
            A.E.edge_of[kb + j] = e;
        } else if (j < cells) A.E.edge_of[kb + j] = -1;
        __syncthreads();
    }
    if (tid == 0) A.E.edge_end[f] = (int32_t)kb + running;
}

__global__ __launch_bounds__(SR_LANES) void k_srk_scatter(SrkDev A)
{
    const int f = blockIdx.y, j = blockIdx.x * SR_LANES + threadIdx.x;
    if (j >= A.cells) return;
    const size_t kb = (size_t)f * A.cells, g = kb + j;
    const uint8_t out = ygz_edge_scatter(A.E, kb, g, A.cells);
    A.prior[g] = out ? -1 : A.kp_point[g];
    if (j == 0 && A.status[f] == 0 && A.inliers[f] < A.min_inliers) A.status[f] = 2;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
extern "C" {

void ygz_hip_default_srk_params(ygz_srk_params *p)
{
    if (!p) return;
    p->baseline = 0.1; p->th_low = 50; p->knn_ratio = 0.7f; p->levelsup = 4; p->check_orientation = 1; p->min_matches = 15; p->min_inliers = 10;
    ygz_hip_default_pose_opt_params(&p->pose);
    p->pose.baseline = p->baseline;
}

int ygz_hip_stereo_ref_keyframe_slots(ygz_hip_ctx *ctx, int n_sets, const ygz_strack_points *sets, int n_keyframes, const int32_t *kf_slot,
                                      const int32_t *kf_set, const int32_t *kf_point, int n_frames, const int32_t *slot, const int32_t *kf,
                                      const double *T, const ygz_srk_params *params, double *T_out, int32_t *status, int32_t *counts,
                                      int32_t *kp_point, int32_t *prior, uint8_t *outlier, double *chi2, int32_t *inliers, int32_t *rounds_run,
                                      int32_t *round_status, int32_t *round_iterations, double *round_cost_initial, double *round_cost_final,
                                      double *round_lambda, int32_t *match12, int32_t *outcome, int32_t *rot)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!sets || !kf_slot || !kf_set || !kf_point || !slot || !kf || !T || !T_out || n_sets < 1 || n_keyframes < 1 || n_frames < 1)
        return YGZ_E_INVALID;
    if (n_sets > YGZ_SRK_MAX_SETS || n_keyframes > YGZ_SRK_MAX_KEYFRAMES || n_frames > YGZ_SRK_MAX_FRAMES) return YGZ_E_CAPACITY;
    ygz_srk_params p;
    if (params) p = *params; else ygz_hip_default_srk_params(&p);
    if (!isfinite(p.baseline) || !isfinite(p.knn_ratio)) return YGZ_E_INVALID;
    if (!(p.baseline > 0) || p.th_low < 0 || p.th_low > 256 || !(p.knn_ratio > 0) || p.levelsup < 0 || p.min_matches < 0 || p.min_inliers < 0)
        return YGZ_E_INVALID;
    if (!ygz_pose_params_ok(p.pose)) return YGZ_E_INVALID;
    for (int s = 0; s < n_sets; ++s)
        if (sets[s].n_pt < 0 || (sets[s].n_pt > 0 && !sets[s].pw)) return YGZ_E_INVALID;
    for (int k = 0; k < n_keyframes; ++k)
        if (kf_slot[k] < 0 || kf_set[k] < 0 || kf_set[k] >= n_sets) return YGZ_E_INVALID;
    for (int f = 0; f < n_frames; ++f)
        if (slot[f] < 0 || kf[f] < 0 || kf[f] >= n_keyframes) return YGZ_E_INVALID;
    const size_t F = (size_t)n_frames, Kn = (size_t)n_keyframes;
    if (!ygz_all_finite(T, 7 * F)) return YGZ_E_INVALID;
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
    const size_t Cn = (size_t)ctx->cells, NK = F * Cn;
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

    // the distinct slots of the call, keyframes first, in the order they first appear; the span of slots k_bow_transform is launched over
    std::vector<int32_t> slots, where((size_t)ctx->prm.max_frames, -1), ds(F), e_off(F);
    for (size_t k = 0; k < Kn; ++k) ygz_distinct_slot(slots, where, kf_slot[k]);
    for (size_t f = 0; f < F; ++f) {
        ds[f] = ygz_distinct_slot(slots, where, slot[f]);
        e_off[f] = (int32_t)(f * Cn);
    }
    int32_t slot_min = slots[0], slot_max = slots[0];
    for (int32_t s : slots) { if (s < slot_min) slot_min = s; if (s > slot_max) slot_max = s; }
    const size_t D = slots.size(), SP = (size_t)(slot_max - slot_min + 1);
    std::vector<int32_t> named(SP, 0);
    for (int32_t s : slots) named[(size_t)(s - slot_min)] = 1;

    // up: [the tables | the sets | kf_point | poses), back: [poses | the small outputs | the per-keypoint outputs), then what stays on the device
    YgzBlobLayout B;
    const size_t o_slots = B.add_n<int32_t>(D), o_named = B.add_n<int32_t>(SP), o_kslot = B.add_n<int32_t>(Kn), o_kset = B.add_n<int32_t>(Kn);
    const size_t o_fslot = B.add_n<int32_t>(F), o_fds = B.add_n<int32_t>(F), o_fkf = B.add_n<int32_t>(F), o_off = B.add_n<int32_t>(F);
    const size_t o_tab = B.add_n<SrkSetTab>((size_t)n_sets);
    std::vector<SrkSetTab> tab((size_t)n_sets);
    for (int s = 0; s < n_sets; ++s) {
        tab[(size_t)s].pw = B.add_n<double>((size_t)sets[s].n_pt * 3);
        tab[(size_t)s].n_pt = sets[s].n_pt; tab[(size_t)s].pad_ = 0;
    }
    const size_t o_kfp = B.add_n<int32_t>(Kn * Cn);
    const size_t o_pose = B.add_n<double>(F * 7), in_end = B.end;
    const size_t o_status = B.add_n<int32_t>(F), o_counts = B.add_n<int32_t>(F * 8);
    YgzPoseBlock PB;
    PB.add_results(B, F);
    const size_t o_rot = B.add_n<int32_t>(F * 33);
    size_t back_end = B.end;
    // the per-keypoint outputs, fetched up to the last one the caller asked for
    const size_t o_prior = B.add_n<int32_t>(NK); if (prior) back_end = B.end;
    const size_t o_kpt = B.add_n<int32_t>(NK); if (kp_point) back_end = B.end;
    const size_t o_out = B.add_n<uint8_t>(NK); if (outlier) back_end = B.end;
    const size_t o_chi2 = B.add_n<double>(NK); if (chi2) back_end = B.end;
    const size_t o_m12 = B.add_n<int32_t>(NK); if (match12) back_end = B.end;
    const size_t o_oc = B.add_n<int32_t>(NK); if (outcome) back_end = B.end;
    const size_t o_hold = B.add_n<int32_t>(NK);
    PB.add_edges(B, F, Cn);
    const size_t o_gur = B.add_n<double>(D * Cn), o_bown = B.add_n<int32_t>(SP), o_node1 = B.add_n<int32_t>(Kn * Cn);
    const size_t o_pairs = B.add_n<BowPair>(F), o_bcnt = B.add_n<int32_t>(F), total = B.end;
    YgzBlob blob;
    int rc = ygz_blob_open(ctx, SCR_SRK, total, back_end, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    memcpy(up + o_slots, slots.data(), D * 4); memcpy(up + o_named, named.data(), SP * 4);
    memcpy(up + o_kslot, kf_slot, Kn * 4); memcpy(up + o_kset, kf_set, Kn * 4);
    memcpy(up + o_fslot, slot, F * 4); memcpy(up + o_fds, ds.data(), F * 4); memcpy(up + o_fkf, kf, F * 4); memcpy(up + o_off, e_off.data(), F * 4);
    memcpy(up + o_tab, tab.data(), (size_t)n_sets * sizeof(SrkSetTab));
    for (int s = 0; s < n_sets; ++s)
        if (sets[s].n_pt > 0) memcpy(up + tab[(size_t)s].pw, sets[s].pw, (size_t)sets[s].n_pt * 24);
    memcpy(up + o_kfp, kf_point, Kn * Cn * 4);
    memcpy(up + o_pose, T, F * 56);
    if ((rc = ygz_blob_upload(ctx, blob, in_end)) != YGZ_OK) return rc;

    const ygz_hip_ctx::Vocab *v = ctx->vocab;
    const double K4[4] = { (double)ctx->prm.fx, (double)ctx->prm.fy, (double)ctx->prm.cx, (double)ctx->prm.cy };
    SrkDev A;
    memset(&A, 0, sizeof A);
    A.kp_px = ctx->kp_px; A.kp_level = ctx->kp_level; A.kp_desc = ctx->kp_desc; A.kp_angle = ctx->kp_angle; A.n_kp = ctx->n_kp;
    A.kp_depth = ctx->kp_depth; A.kp_has_mp = ctx->kp_has_mp; A.kp_node = v->kp_node;
    A.block = dev; A.set_tab = ygz_at<const SrkSetTab>(dev, o_tab);
    A.slots = ygz_at<const int32_t>(dev, o_slots); A.named = ygz_at<const int32_t>(dev, o_named);
    A.kf_slot = ygz_at<const int32_t>(dev, o_kslot); A.kf_set = ygz_at<const int32_t>(dev, o_kset); A.kf_point = ygz_at<const int32_t>(dev, o_kfp);
    A.fr_slot = ygz_at<const int32_t>(dev, o_fslot); A.fr_dslot = ygz_at<const int32_t>(dev, o_fds); A.fr_kf = ygz_at<const int32_t>(dev, o_fkf);
    A.g_ur = ygz_at<double>(dev, o_gur); A.bow_n = ygz_at<int32_t>(dev, o_bown); A.node1 = ygz_at<int32_t>(dev, o_node1);
    A.pairs = ygz_at<BowPair>(dev, o_pairs); A.bow_cnt = ygz_at<int32_t>(dev, o_bcnt);
    A.match12 = ygz_at<int32_t>(dev, o_m12); A.outcome = ygz_at<int32_t>(dev, o_oc);
    A.holder = ygz_at<int32_t>(dev, o_hold); A.kp_point = ygz_at<int32_t>(dev, o_kpt); A.prior = ygz_at<int32_t>(dev, o_prior);
    ygz_slot_edges_bind(A.E, dev, PB, o_out, o_chi2);
    A.status = ygz_at<int32_t>(dev, o_status); A.counts = ygz_at<int32_t>(dev, o_counts);
    A.rot = ygz_at<int32_t>(dev, o_rot); A.inliers = ygz_at<const int32_t>(dev, PB.inliers);
    A.bf = K4[0] * p.baseline;
    A.cells = ctx->cells; A.n_frames = n_frames; A.n_slots = (int)D; A.n_kf = n_keyframes; A.slot_min = slot_min; A.span = (int)SP;
    A.check_orientation = p.check_orientation ? 1 : 0; A.min_matches = p.min_matches; A.min_inliers = p.min_inliers;

    VocDev V;
    V.L = v->L; V.child_off = v->child_off; V.child = v->child; V.word_id = v->word_id; V.desc = v->desc; V.weight = v->weight;

    PoptArgs G;
    memset(&G, 0, sizeof G);
    ygz_popt_bind(G, dev, PB, o_off, o_pose);
    ygz_popt_set_params(G, K4, p.baseline, p.pose);

    int widest = ctx->cells > n_frames ? ctx->cells : n_frames;
    if ((int)SP > widest) widest = (int)SP;
    const unsigned bx = (unsigned)ygz_div_up(ctx->cells, SR_LANES), bt = (unsigned)ygz_div_up(widest, SR_LANES);
    const size_t so = (size_t)slot_min * Cn;
    YGZ_LAUNCH(ctx, KID_SRK_GATHER, k_srk_gather, dim3(bt, (unsigned)D), dim3(SR_LANES), A, 0);
    YGZ_LAUNCH(ctx, KID_BOW_TRANSFORM, k_bow_transform, dim3(bx, (unsigned)SP), dim3(256), V, ctx->kp_desc + 8 * so, (const int32_t *)A.bow_n, 0, Cn,
               p.levelsup, v->kp_word + so, v->kp_weight + so, v->kp_node + so);
    YGZ_LAUNCH(ctx, KID_SRK_GATHER, k_srk_gather, dim3(bx, (unsigned)n_keyframes), dim3(SR_LANES), A, 1);
    YGZ_LAUNCH(ctx, KID_BOW_MATCH, k_bow_match<0>, dim3(bx, (unsigned)n_frames), dim3(256), (const BowPair *)A.pairs, (int)p.th_low, p.knn_ratio, 0.0,
               K4[0], K4[1], K4[2], K4[3], A.match12, Cn, A.bow_cnt);
    YGZ_LAUNCH(ctx, KID_SRK_RESOLVE, k_srk_resolve, dim3((unsigned)n_frames), dim3(SR_LANES), A);
    YGZ_LAUNCH(ctx, KID_POSE_OPT, k_pose_opt, dim3((unsigned)n_frames), dim3(PT_DEV_THREADS), G);
    YGZ_LAUNCH(ctx, KID_SRK_SCATTER, k_srk_scatter, dim3(bx, (unsigned)n_frames), dim3(SR_LANES), A);
    if ((rc = ygz_blob_fetch(ctx, blob, o_pose, back_end)) != YGZ_OK) return rc;
    memcpy(T_out, up + o_pose, F * 56);
    if (status) memcpy(status, up + o_status, F * 4);
    if (counts) memcpy(counts, up + o_counts, F * 32);
    PB.copy_results(up, F, inliers, rounds_run, round_status, round_iterations, round_cost_initial, round_cost_final, round_lambda);
    if (rot) memcpy(rot, up + o_rot, F * 132);
    if (prior) memcpy(prior, up + o_prior, NK * 4);
    if (kp_point) memcpy(kp_point, up + o_kpt, NK * 4);
    if (outlier) memcpy(outlier, up + o_out, NK);
    if (chi2) memcpy(chi2, up + o_chi2, NK * 8);
    if (match12) memcpy(match12, up + o_m12, NK * 4);
    if (outcome) memcpy(outcome, up + o_oc, NK * 4);
    return YGZ_OK;
}

}  // extern "C"
