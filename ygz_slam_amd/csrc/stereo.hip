// S0 -- stereo input: the depth of every left keypoint from a rectified pair (the four steps of ORB-SLAM2's Frame::ComputeStereoMatches: row-band
// descriptor search, 11 x 11 SAD search over +-5 columns at the keypoint's level, parabola fit, median rule).  The frozen spec is
// tests/stereo_ref.c: integer work plus a few uncontracted FP64 operations per keypoint, and every output is bit-identical
// to it.
//   k_stereo_match    all pairs in one launch, one wavefront (= one workgroup) per left keypoint: the lanes stride over the pair's right keypoints
//                     (level, row band, u range, then the 256-bit Hamming distance), the minimum of (dist << 22 | j) is a wave reduction; the left
//                     patch (121 bytes) and the right strip (11 x 21 bytes) are staged in LDS, the 11 sums are integer wave reductions, and the
//                     FP64 tail is the same in every lane (lane 0 writes)
//   k_stereo_median   one workgroup per pair: element m / 2 of the OK keypoints' sorted SAD values by a two-pass radix select (two 256-bin LDS
//                     histograms of 16-bit values), then the rule, the counts and -- when asked -- the left slot's depths
// Integer reductions and integer LDS counters only: no output depends on scheduling.  No wait for another workgroup, no scratch, no environment
// switch; every image address lies inside the picture by the border test of step 5.
#include "ygz_internal.h"
#include <math.h>
#include <string.h>
#include <vector>
#pragma clang fp contract(off)

#define ST_W 5                    // patch half-size
#define ST_L 5                    // search half-range
#define ST_P (2 * ST_W + 1)       // 11: patch side
#define ST_N (2 * ST_L + 1)       // 11: columns searched
#define ST_SW (ST_P + ST_N - 1)   // 21: width of the right strip
#define ST_JBITS 22               // (dist << 22 | j): dist <= 256, j < 2^22
#define ST_TAB 6                  // ints per pair of the pair table

struct StereoArgs {
    const int32_t *tab;           // [n_pairs][6]: image slot L, R; keypoint set L, R; nL, nR (< 0: the set's resident count n_kp[set])
    const int32_t *n_kp;
    const double *px; const int32_t *level; const uint32_t *desc;      // keypoint sets: set s at s * kp_stride (px x 2, desc x 8)
    int kp_stride, out_stride, n_levels, th_dist;
    const uint8_t *lvl[YGZ_MAX_LEVELS]; int lw[YGZ_MAX_LEVELS], lh[YGZ_MAX_LEVELS];
    double bf, minD, maxD;
    int32_t *right_idx, *sad, *status, *counts;                        // [n_pairs][out_stride], counts [n_pairs][7]
    double *u_right, *depth;
    int32_t *best_idx, *best_dist, *n_cand, *sads;                     // the stage for tests (nullptr: not wanted); sads [..][11]
    double *kp_depth; uint8_t *kp_has_mp;                              // != nullptr: the left set's depths are written (stride kp_stride)
};

__device__ __forceinline__ int st_count(const StereoArgs &A, const int32_t *t, int side)
{
    const int n = t[4 + side];
    return n >= 0 ? n : A.n_kp[t[2 + side]];
}

__global__ __launch_bounds__(64) void k_stereo_match(StereoArgs A)
{
    __shared__ uint8_t s_left[ST_P * ST_P + 7];
    __shared__ uint8_t s_right[ST_P * ST_SW + 1];
    const int pair = (int)blockIdx.y, i = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int32_t *t = A.tab + ST_TAB * pair;
    const int nL = st_count(A, t, 0), nR = st_count(A, t, 1);
    const size_t o = (size_t)pair * A.out_stride + i;
    int status = YGZ_STEREO_NO_CANDIDATE, bj = -1, bd = -1, nc = 0, d2 = -1, reached = 0;
    int D[ST_N];
    double uRs = -1.0, depth = -1.0;
    if (i >= nL) status = -1;                                          // past the pair's left keypoints: every output is -1
    else {
        const size_t kl = (size_t)t[2] * A.kp_stride + i, kr0 = (size_t)t[3] * A.kp_stride;
        const double uL = A.px[2 * kl], vL = A.px[2 * kl + 1];
        const int l = A.level[kl];
        // steps 1-3: the lanes stride over the right keypoints
        uint32_t best = 0xFFFFFFFFu;
        if (!(uL - A.minD < 0.0) && (unsigned)l < (unsigned)A.n_levels) {
            uint32_t dl[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) dl[k] = A.desc[8 * kl + k];
            const double lo = uL - A.maxD, hi = uL - A.minD, fvL = floor(vL);
            // a row that the band test can admit lies within r + 2 of vL, and r <= 4 * 2^l because |lr - l| <= 1: the 8 bytes of vR turn most
            // right keypoints away before their level and column are read (a superset of the exact test below, which decides)
            const double reach = (double)(4 << l) + 3.0, v_lo = vL - reach, v_hi = vL + reach;
            for (int j = lane; j < nR; j += 64) {
                const double vR = A.px[2 * (kr0 + j) + 1];
                if (vR < v_lo || vR > v_hi) continue;
                const int lr = A.level[kr0 + j];
                if (lr - l > 1 || l - lr > 1) continue;
                const double uR = A.px[2 * (kr0 + j)];
                const double r = 2.0 * (double)(1 << lr);
                if (!(floor(vR - r) <= fvL && fvL <= ceil(vR + r))) continue;
                if (!(uR >= lo && uR <= hi)) continue;
                ++nc;
                const uint4 a = *reinterpret_cast<const uint4 *>(A.desc + 8 * (kr0 + j)), b = *reinterpret_cast<const uint4 *>(A.desc + 8 * (kr0 + j) + 4);
                const int d = __popc(a.x ^ dl[0]) + __popc(a.y ^ dl[1]) + __popc(a.z ^ dl[2]) + __popc(a.w ^ dl[3]) +
                              __popc(b.x ^ dl[4]) + __popc(b.y ^ dl[5]) + __popc(b.z ^ dl[6]) + __popc(b.w ^ dl[7]);
                best = min(best, ((uint32_t)d << ST_JBITS) | (uint32_t)j);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, m));
        best = (uint32_t)__builtin_amdgcn_readfirstlane((int)best);
        nc = ygz_wave_sum_i(nc);
        if (best != 0xFFFFFFFFu) {
            bj = (int)(best & ((1u << ST_JBITS) - 1u)); bd = (int)(best >> ST_JBITS);
            if (bd >= A.th_dist) status = YGZ_STEREO_DESCRIPTOR;
            else {
                // steps 4, 5: the three columns at the keypoint's level (a division by a power of two is exact)
                const double s = (double)(1 << l);
                const int su = (int)floor(uL / s + 0.5), sv = (int)floor(vL / s + 0.5), sr = (int)floor(A.px[2 * (kr0 + bj)] / s + 0.5);
                int Wl = 0, Hl = 0;
                const uint8_t *base = nullptr;
#pragma unroll
                for (int k = 0; k < YGZ_MAX_LEVELS; ++k) if (k == l) { Wl = A.lw[k]; Hl = A.lh[k]; base = A.lvl[k]; }
                if (!(ST_W <= su && su < Wl - ST_W && ST_W <= sv && sv < Hl - ST_W && sr - ST_L - ST_W >= 0 && sr + ST_L + ST_W < Wl)) status = YGZ_STEREO_BORDER;
                else {
                    // step 6: rows sv - 5 .. sv + 5 of both pictures, columns su - 5 .. su + 5 and sr - 10 .. sr + 10: inside by step 5
                    const size_t plane = (size_t)Wl * Hl;
                    const uint8_t *IL = base + (size_t)t[0] * plane + (size_t)(sv - ST_W) * Wl + (su - ST_W);
                    const uint8_t *IR = base + (size_t)t[1] * plane + (size_t)(sv - ST_W) * Wl + (sr - ST_L - ST_W);
                    for (int p = lane; p < ST_P * ST_P; p += 64) s_left[p] = IL[(size_t)(p / ST_P) * Wl + (p % ST_P)];
                    for (int q = lane; q < ST_P * ST_SW; q += 64) s_right[q] = IR[(size_t)(q / ST_SW) * Wl + (q % ST_SW)];
                    __syncthreads();                                   // the whole workgroup is this wavefront, and the branch is uniform over it
                    const int cL = s_left[ST_W * ST_P + ST_W];
                    int cR[ST_N];
#pragma unroll
                    for (int q = 0; q < ST_N; ++q) { cR[q] = s_right[ST_W * ST_SW + ST_W + q]; D[q] = 0; }
                    for (int p = lane; p < ST_P * ST_P; p += 64) {
                        const int dy = p / ST_P, dx = p % ST_P;
                        const int a = (int)s_left[p] - cL;
#pragma unroll
                        for (int q = 0; q < ST_N; ++q) {
                            const int b = (int)s_right[dy * ST_SW + dx + q] - cR[q];
                            D[q] += a > b ? a - b : b - a;
                        }
                    }
                    int k = 0, dmin = 0x7FFFFFFF;
#pragma unroll
                    for (int q = 0; q < ST_N; ++q) { D[q] = ygz_wave_sum_i(D[q]); if (D[q] < dmin) { dmin = D[q]; k = q; } }
                    reached = 1;
                    // steps 7-10, the same in every lane
                    if (k == 0 || k == ST_N - 1) status = YGZ_STEREO_EDGE;
                    else {
                        int d1 = 0, d3 = 0;
#pragma unroll
                        for (int q = 1; q < ST_N - 1; ++q) if (q == k) { d1 = D[q - 1]; d3 = D[q + 1]; }
                        const int den = d1 + d3 - 2 * dmin;
                        const double delta = (double)(d1 - d3) / (double)(2 * den);
                        double ur = s * ((double)(sr + k - ST_L) + delta);
                        double disp = uL - ur;
                        if (!(disp >= A.minD && disp < A.maxD)) status = YGZ_STEREO_DISPARITY;
                        else {
                            if (disp <= 0.0) { disp = 0.01; ur = uL - 0.01; }
                            status = YGZ_STEREO_OK; uRs = ur; depth = A.bf / disp; d2 = dmin;
                        }
                    }
                }
            }
        }
    }
    if (lane == 0) {
        A.status[o] = status;
        A.right_idx[o] = status == YGZ_STEREO_OK ? bj : -1;
        A.sad[o] = d2; A.u_right[o] = uRs; A.depth[o] = depth;
        if (A.best_idx) { A.best_idx[o] = bj; A.best_dist[o] = bd; A.n_cand[o] = status < 0 ? -1 : nc; }
    }
    if (A.sads && lane < ST_N) {
        int v = -1;
#pragma unroll
        for (int q = 0; q < ST_N; ++q) if (q == lane && reached) v = D[q];
        A.sads[o * ST_N + lane] = v;
    }
}

__global__ __launch_bounds__(256) void k_stereo_median(StereoArgs A)
{
    __shared__ unsigned s_hist[256];
    __shared__ int s_cnt[YGZ_STEREO_N_STATUS];
    __shared__ int s_sel[3];                                           // m, the bin chosen, the rank inside it
    const int pair = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int32_t *t = A.tab + ST_TAB * pair;
    const int nL = st_count(A, t, 0);
    const size_t o = (size_t)pair * A.out_stride;
    int med = 0;
    for (int pass = 0; pass < 2; ++pass) {
        s_hist[tid] = 0;
        if (tid < YGZ_STEREO_N_STATUS) s_cnt[tid] = 0;
        __syncthreads();
        const int m0 = s_sel[0], bin = s_sel[1];                       // of pass 0 (read by pass 1 only)
        if (pass == 0 || m0 > 0)
            for (int i = tid; i < nL; i += 256)
                if (A.status[o + i] == YGZ_STEREO_OK) {
                    const int v = A.sad[o + i];
                    if (pass == 0) atomicAdd(&s_hist[(v >> 8) & 255], 1u);
                    else if (((v >> 8) & 255) == bin) atomicAdd(&s_hist[v & 255], 1u);
                }
        __syncthreads();
        if (tid == 0) {
            int m = 0;
            if (pass == 0) { for (int b = 0; b < 256; ++b) m += (int)s_hist[b]; s_sel[0] = m; }
            int rank = pass == 0 ? m / 2 : s_sel[2], b = 0, cum = 0;
            if (pass == 0 ? m > 0 : m0 > 0) {
                for (; b < 255 && cum + (int)s_hist[b] <= rank; ++b) cum += (int)s_hist[b];
                s_sel[1] = pass == 0 ? b : (bin << 8 | b);
                s_sel[2] = rank - cum;
            }
        }
        __syncthreads();
    }
    const int m = s_sel[0];
    med = s_sel[1];
    __syncthreads();
    for (int i = tid; i < nL; i += 256) {
        int st = A.status[o + i];
        double dp = A.depth[o + i];
        if (st == YGZ_STEREO_OK && m > 0 && 10ll * (long long)A.sad[o + i] > 21ll * (long long)med) {
            st = YGZ_STEREO_MEDIAN; dp = -1.0;
            A.status[o + i] = st; A.depth[o + i] = dp; A.u_right[o + i] = -1.0;
        }
        atomicAdd(&s_cnt[st], 1);
        if (A.kp_depth) {
            const size_t kl = (size_t)t[2] * A.kp_stride + i;
            A.kp_depth[kl] = dp; A.kp_has_mp[kl] = st == YGZ_STEREO_OK ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid < YGZ_STEREO_N_STATUS) A.counts[(size_t)pair * YGZ_STEREO_N_STATUS + tid] = s_cnt[tid];
}

static bool stereo_params_ok(const ygz_stereo_params &p)
{
    if (!isfinite(p.baseline) || !isfinite(p.min_disparity) || !isfinite(p.max_disparity)) return false;
    return p.baseline > 0.0 && p.min_disparity >= 0.0 && p.max_disparity >= 0.0 && p.th_dist >= 0 && p.th_dist <= 256;
}

struct StereoHostOut {          // the caller's arrays, [n_pairs][stride] (counts [n_pairs][7]); any may be nullptr
    int32_t *right_idx; double *u_right, *depth; int32_t *sad, *status, *counts;
    int32_t *best_idx, *best_dist, *n_cand, *sads;
};
struct StereoHostKp { const double *px; const int32_t *level; const uint8_t *desc; int n; };

// One call: the pair table (and, in the array form, the two keypoint lists behind it) in ONE upload, the two launches, ONE copy back, one wait.
// kp == nullptr: the resident keypoints of the slots; else kp[0], kp[1] are the left and the right list of the ONE pair (sets 0 and 1).
static int stereo_run(ygz_hip_ctx *ctx, int n_pairs, const int32_t *left_slot, const int32_t *right_slot, const StereoHostKp *kp,
                      const ygz_stereo_params &p, bool stage_outputs, bool write_depths, const StereoHostOut &out)
{
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (write_depths) { int rc = ygz_track_ensure(ctx); if (rc != YGZ_OK) return rc; }
    const size_t cells = (size_t)ctx->cells;
    const size_t stride = kp ? (size_t)(kp[0].n > 0 ? kp[0].n : 1) : cells, kp_stride = kp ? (size_t)(kp[0].n > kp[1].n ? kp[0].n : kp[1].n) : cells;
    const size_t N = (size_t)n_pairs * stride;
    // up: [table | px | level | desc), back: [u_right | depth | right_idx | sad | status | counts | best_idx | best_dist | n_cand | sads).
    // Every array at a multiple of 256 bytes, as in every packed block (this file aligned to 64 before: the block grows by a few KB, no output changes)
    YgzBlobLayout L;
    const size_t KP = kp ? 2 * kp_stride : 0, NS = stage_outputs ? N : 0;          // absent arrays take no room
    const size_t o_tab = L.add_n<int32_t>((size_t)n_pairs * ST_TAB);
    const size_t o_px = L.add_n<double>(KP * 2), o_lv = L.add_n<int32_t>(KP), o_ds = L.add_n<uint32_t>(KP * 8), in_end = L.end;
    const size_t o_ur = L.add_n<double>(N), o_dp = L.add_n<double>(N), o_ri = L.add_n<int32_t>(N), o_sd = L.add_n<int32_t>(N);
    const size_t o_st = L.add_n<int32_t>(N), o_ct = L.add_n<int32_t>((size_t)n_pairs * YGZ_STEREO_N_STATUS);
    const size_t o_bi = L.add_n<int32_t>(NS), o_bd = L.add_n<int32_t>(NS), o_nc = L.add_n<int32_t>(NS), o_ss = L.add_n<int32_t>(NS * ST_N);
    const size_t total = L.end;
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_STEREO, total, total, &b);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = b.host, *dev = b.dev;
    int32_t *tab = ygz_at<int32_t>(up, o_tab);
    for (int q = 0; q < n_pairs; ++q) {
        int32_t *e = tab + ST_TAB * q;
        e[0] = left_slot[q]; e[1] = right_slot[q];
        e[2] = kp ? 0 : left_slot[q]; e[3] = kp ? 1 : right_slot[q];
        e[4] = kp ? kp[0].n : -1; e[5] = kp ? kp[1].n : -1;
    }
    if (kp)
        for (int s = 0; s < 2; ++s) {
            const size_t n = (size_t)kp[s].n;
            if (!n) continue;
            memcpy(up + o_px + s * kp_stride * 16, kp[s].px, n * 16);
            memcpy(up + o_lv + s * kp_stride * 4, kp[s].level, n * 4);
            memcpy(up + o_ds + s * kp_stride * 32, kp[s].desc, n * 32);
        }
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    StereoArgs A;
    memset(&A, 0, sizeof(A));
    A.tab = ygz_at<const int32_t>(dev, o_tab); A.n_kp = ctx->n_kp;
    A.px = kp ? ygz_at<const double>(dev, o_px) : ctx->kp_px; A.level = kp ? ygz_at<const int32_t>(dev, o_lv) : ctx->kp_level;
    A.desc = kp ? ygz_at<const uint32_t>(dev, o_ds) : ctx->kp_desc;
    A.kp_stride = (int)kp_stride; A.out_stride = (int)stride; A.n_levels = ctx->prm.pyramid_levels; A.th_dist = p.th_dist;
    for (int l = 0; l < ctx->prm.pyramid_levels; ++l) { A.lvl[l] = ctx->lvl[l]; A.lw[l] = ctx->lw[l]; A.lh[l] = ctx->lh[l]; }
    const double fx_d = (double)ctx->prm.fx;
    A.bf = fx_d * p.baseline; A.minD = p.min_disparity; A.maxD = p.max_disparity == 0.0 ? fx_d : p.max_disparity;
    A.u_right = ygz_at<double>(dev, o_ur); A.depth = ygz_at<double>(dev, o_dp); A.right_idx = ygz_at<int32_t>(dev, o_ri);
    A.sad = ygz_at<int32_t>(dev, o_sd); A.status = ygz_at<int32_t>(dev, o_st); A.counts = ygz_at<int32_t>(dev, o_ct);
    if (stage_outputs) {
        A.best_idx = ygz_at<int32_t>(dev, o_bi); A.best_dist = ygz_at<int32_t>(dev, o_bd); A.n_cand = ygz_at<int32_t>(dev, o_nc);
        A.sads = ygz_at<int32_t>(dev, o_ss);
    }
    if (write_depths) { A.kp_depth = ctx->kp_depth; A.kp_has_mp = ctx->kp_has_mp; }
    YGZ_LAUNCH(ctx, KID_STEREO_MATCH, k_stereo_match, dim3((unsigned)stride, (unsigned)n_pairs), dim3(64), A);
    YGZ_HIPCHK(ctx, hipGetLastError());
    YGZ_LAUNCH(ctx, KID_STEREO_MEDIAN, k_stereo_median, dim3((unsigned)n_pairs), dim3(256), A);
    if ((rc = ygz_blob_fetch(ctx, b, in_end, total)) != YGZ_OK) return rc;
    const size_t n_out = kp ? (size_t)kp[0].n : N;
    if (out.u_right) memcpy(out.u_right, up + o_ur, n_out * 8);
    if (out.depth) memcpy(out.depth, up + o_dp, n_out * 8);
    if (out.right_idx) memcpy(out.right_idx, up + o_ri, n_out * 4);
    if (out.sad) memcpy(out.sad, up + o_sd, n_out * 4);
    if (out.status) memcpy(out.status, up + o_st, n_out * 4);
    if (out.counts) memcpy(out.counts, up + o_ct, (size_t)n_pairs * YGZ_STEREO_N_STATUS * 4);
    if (stage_outputs) {
        if (out.best_idx) memcpy(out.best_idx, up + o_bi, n_out * 4);
        if (out.best_dist) memcpy(out.best_dist, up + o_bd, n_out * 4);
        if (out.n_cand) memcpy(out.n_cand, up + o_nc, n_out * 4);
        if (out.sads) memcpy(out.sads, up + o_ss, n_out * ST_N * 4);
    }
    return YGZ_OK;
}

// the checks of the array form that need no device: YGZ_OK or the error
static int stereo_check_arrays(const ygz_hip_ctx *ctx, int left_slot, int right_slot, const StereoHostKp kp[2], const ygz_stereo_params *params)
{
    if (!params || kp[0].n < 0 || kp[1].n < 0) return YGZ_E_INVALID;
    for (int s = 0; s < 2; ++s) if (kp[s].n > 0 && (!kp[s].px || !kp[s].level || !kp[s].desc)) return YGZ_E_INVALID;
    if (!stereo_params_ok(*params) || left_slot < 0 || right_slot < 0 || left_slot == right_slot) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    if (left_slot >= ctx->prm.max_frames || right_slot >= ctx->prm.max_frames) return YGZ_E_INVALID;
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < kp[s].n; ++i) if (kp[s].level[i] < 0 || kp[s].level[i] >= ctx->prm.pyramid_levels) return YGZ_E_INVALID;
    if (kp[0].n > ctx->cells || kp[1].n > ctx->cells || ctx->cells > (1 << ST_JBITS)) return YGZ_E_CAPACITY;
    if (!ctx->pyr_valid[left_slot] || !ctx->pyr_valid[right_slot]) return YGZ_E_STATE;
    return YGZ_OK;
}

extern "C" {

void ygz_hip_default_stereo_params(ygz_stereo_params *p)
{
    if (!p) return;
    p->baseline = 0.1; p->min_disparity = 0.0; p->max_disparity = 0.0; p->th_dist = 75; p->write_depths = 1;
}

int ygz_hip_stereo_depths_slots(ygz_hip_ctx *ctx, int n_pairs, const int32_t *left_slot, const int32_t *right_slot, const ygz_stereo_params *params,
                                int32_t *right_idx, double *u_right, double *depth, int32_t *sad, int32_t *status, int32_t *counts)
{
    if (!params || !left_slot || !right_slot || n_pairs < 1 || !stereo_params_ok(*params)) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    std::vector<uint8_t> named((size_t)ctx->prm.max_frames, 0);
    for (int q = 0; q < n_pairs; ++q) {
        const int a = left_slot[q], b = right_slot[q];
        if (a < 0 || a >= ctx->prm.max_frames || b < 0 || b >= ctx->prm.max_frames || a == b || named[a]) return YGZ_E_INVALID;
        named[a] = 1;
    }
    if (ctx->cells > (1 << ST_JBITS)) return YGZ_E_CAPACITY;
    for (int q = 0; q < n_pairs; ++q) {
        const int a = left_slot[q], b = right_slot[q];
        if (!ctx->pyr_valid[a] || !ctx->pyr_valid[b] || !ctx->kp_valid[a] || !ctx->kp_valid[b]) return YGZ_E_STATE;
    }
    const StereoHostOut out = { right_idx, u_right, depth, sad, status, counts, nullptr, nullptr, nullptr, nullptr };
    return stereo_run(ctx, n_pairs, left_slot, right_slot, nullptr, *params, false, params->write_depths != 0, out);
}

int ygz_hip_stereo_match(ygz_hip_ctx *ctx, int left_slot, int right_slot, const double *px_l, const int32_t *level_l, const uint8_t *desc_l, int n_l,
                         const double *px_r, const int32_t *level_r, const uint8_t *desc_r, int n_r, const ygz_stereo_params *params,
                         int32_t *right_idx, double *u_right, double *depth, int32_t *sad, int32_t *status, int32_t *counts)
{
    const StereoHostKp kp[2] = { { px_l, level_l, desc_l, n_l }, { px_r, level_r, desc_r, n_r } };
    const int rv = stereo_check_arrays(ctx, left_slot, right_slot, kp, params);
    if (rv != YGZ_OK) return rv;
    if (n_l == 0) {                                                     // nothing to match: no launch
        if (counts) memset(counts, 0, YGZ_STEREO_N_STATUS * 4);
        return YGZ_OK;
    }
    const int32_t ls = left_slot, rs = right_slot;
    const StereoHostOut out = { right_idx, u_right, depth, sad, status, counts, nullptr, nullptr, nullptr, nullptr };
    return stereo_run(ctx, 1, &ls, &rs, kp, *params, false, false, out);
}

int ygz_hip_stereo_candidates(ygz_hip_ctx *ctx, int left_slot, int right_slot, const double *px_l, const int32_t *level_l, const uint8_t *desc_l, int n_l,
                              const double *px_r, const int32_t *level_r, const uint8_t *desc_r, int n_r, const ygz_stereo_params *params,
                              int32_t *best_idx, int32_t *best_dist, int32_t *n_cand, int32_t *sads)
{
    const StereoHostKp kp[2] = { { px_l, level_l, desc_l, n_l }, { px_r, level_r, desc_r, n_r } };
    const int rv = stereo_check_arrays(ctx, left_slot, right_slot, kp, params);
    if (rv != YGZ_OK) return rv;
    if (n_l == 0) return YGZ_OK;
    const int32_t ls = left_slot, rs = right_slot;
    const StereoHostOut out = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, best_idx, best_dist, n_cand, sads };
    return stereo_run(ctx, 1, &ls, &rs, kp, *params, true, false, out);
}

}  // extern "C"
