// Local-map selection: ORB-SLAM2's Tracking::UpdateLocalKeyFrames in StereoTracker::LocalKeyFrames' form (no spanning tree) and
// UpdateLocalPoints, for many frames on one map in one call.  The map is ygz_hip_covisibility's point-major CSR with the
// feature index of every observation; on the device an observation is ONE word, keyframe | feature << 16.
//
//   k_lms_vote    one workgroup per frame.  The K votes sit in LDS as integers: lanes stride over the frame's entries and their observation
//                 lists with LDS atomicAdd (integer sums are order-free).  The reference keyframe is ONE LDS atomicMax per lane on
//                 vote << 12 | 4095 - k (the largest vote, then the smallest index).  The voters are compacted in index order by ballot and
//                 scan, 256 keyframes a step.  The extension is the one serial part, at most max_keyframes steps because it only runs while
//                 the list is short: the covisible rows of eight voters at a time are staged in LDS with their bad entries struck out, then
//                 per voter the first wavefront looks at the row, a lane per entry, membership from the rank table in LDS, one ballot, first
//                 set bit.  Writes votes, ref, n_voters, n_local, local_kf and the rank table (16 bit, 0xFFFF for none).
//   k_lms_points  grid (rank, frame): stages the frame's rank table in LDS and walks keyframe local_kf[f][r]'s (feature, point) pairs of the
//                 keyframe-major index in order.  A pair is kept exactly when the smallest rank over its point's observers is r: that observer
//                 is this observation, since a point's list holds a keyframe once.  One count per (frame, rank).
//   k_lms_place   same grid: every workgroup of a frame scans the frame's counts over the ranks, walks its keyframes again and writes the kept
//                 points at the offsets, cut at max_points, with the feature index beside them; the first workgroup of a frame writes the
//                 scan, n_pt, n_cut and the padding.
//   k_lms_prior   a lane per frame entry: the smallest rank over the point's observers and that observation's feature give the point's key;
//                 a binary search in that rank's slice of the kept list gives its position.
//
// Integers only: every output is independent of the order the lanes arrive in.  No atomics on global memory, no wait for another workgroup,
// no scratch memory.  The arithmetic is that of tests/lms_ref.c, bit for bit.  Every index a kernel forms was validated by the entry point.
#include "ygz_internal.h"
#include "lms_index.h"
#include "lms_dev.h"
#include <algorithm>
#include <string.h>
#pragma clang fp contract(off)

#define SCR_LMS 46                               // the packed block of ygz_hip_local_map_select: behind srl.hip's 45, inside the context's table
static_assert(SCR_LMS < YGZ_N_SCRATCH, "ygz_hip_ctx::scratch holds the id");
static_assert(YGZ_LMS_FEAT_END == YGZ_LMS_MAX_FEATURES, "the index builder counts over every feature index the call admits");

namespace {

#define LMS_LANES 256
#define LMS_WAVES (LMS_LANES / 64)
#define LMS_ROW   32                             // = YGZ_LMS_MAX_COV: the stride of a staged covisible row
#define LMS_STAGE (LMS_LANES / LMS_ROW)          // voters whose rows are staged at once
#define LMS_NONE  0xFFFF
#define LMS_GRID_RANKS 256                       // workgroups a frame's ranks are dealt to
static_assert(YGZ_LMS_MAX_COV == LMS_ROW && YGZ_LMS_MAX_KEYFRAMES <= 4096, "a rank fits the 12 bits under the vote");

// the position of a set flag among the workgroup's flags in lane order, and their number; two barriers
__device__ __forceinline__ int lms_block_rank(bool flag, int32_t *s_w, int *total)
{
    const unsigned long long b = __ballot(flag);
    const int lane = ygz_lane(), wave = (int)threadIdx.x >> 6;
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < LMS_WAVES; ++w) { const int c = s_w[w]; off += w < wave ? c : 0; tot += c; }
    __syncthreads();
    *total = tot;
    return off + __popcll(b & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ void lms_stage_rank(const LmsDev &A, int f, uint16_t *s_rank)
{
    for (int k = (int)threadIdx.x; k < A.K; k += LMS_LANES) s_rank[k] = A.rank[(size_t)f * A.K + k];
    __syncthreads();
}

// the smallest rank over the observers of point p (LMS_NONE without a local one) and the feature index of that observation
__device__ __forceinline__ int lms_first_rank(const LmsDev &A, const uint16_t *s_rank, int p, int *feat)
{
    int best = LMS_NONE, ft = 0;
    for (int g = A.offsets[p]; g < A.offsets[p + 1]; ++g) {
        const int w = A.obs[g], r = s_rank[w & 0xFFFF];
        if (r < best) { best = r; ft = w >> 16; }
    }
    *feat = ft;
    return best;
}

__global__ __launch_bounds__(LMS_LANES) void k_lms_vote(LmsDev A)
{
    __shared__ int32_t s_votes[YGZ_LMS_MAX_KEYFRAMES];
    __shared__ uint16_t s_rank[YGZ_LMS_MAX_KEYFRAMES], s_list[YGZ_LMS_MAX_KEYFRAMES];
    __shared__ int32_t s_cov[LMS_LANES], s_w[LMS_WAVES], s_best, s_pick;
    const int tid = (int)threadIdx.x, f = (int)blockIdx.x, K = A.K;
    for (int k = tid; k < K; k += LMS_LANES) { s_votes[k] = 0; s_rank[k] = LMS_NONE; }
    if (tid == 0) s_best = 0;
    __syncthreads();
    for (int e = A.fr_off[f] + tid; e < A.fr_off[f + 1]; e += LMS_LANES) {
        const int p = A.fr_pt[e];
        if (p < 0 || A.pt_bad[p]) continue;
        for (int g = A.offsets[p]; g < A.offsets[p + 1]; ++g) atomicAdd(&s_votes[A.obs[g] & 0xFFFF], 1);
    }
    __syncthreads();
    int best = 0;
    for (int k = tid; k < K; k += LMS_LANES) {
        const int v = s_votes[k];
        A.votes[(size_t)f * K + k] = v;
        if (v > 0) best = max(best, (v << 12) | (4095 - k));                      // a vote is at most 32768 = 2^15
    }
    if (best) atomicMax(&s_best, best);
    // the voters in index order
    int n = 0;
    for (int base = 0; base < K; base += LMS_LANES) {
        const int k = base + tid;
        const bool voter = k < K && s_votes[k] > 0 && A.kf_bad[k] == 0;
        int tot;
        const int pos = n + lms_block_rank(voter, s_w, &tot);
        if (voter) { s_rank[k] = (uint16_t)pos; s_list[pos] = (uint16_t)k; }
        n += tot;
    }
    __syncthreads();
    const int voters = n;
    // the extension: n, and with it every loop bound, is the same in every lane
    for (int i0 = 0; i0 < voters && n < A.max_kf; i0 += LMS_STAGE) {
        const int vi = i0 + tid / LMS_ROW, j = tid % LMS_ROW;
        int c = -1;
        if (vi < voters && j < A.C) {
            c = A.cov[(size_t)s_list[vi] * A.C + j];
            if (c >= 0 && A.kf_bad[c]) c = -1;
        }
        s_cov[tid] = c;
        __syncthreads();
        for (int s = 0; s < LMS_STAGE && i0 + s < voters && n < A.max_kf; ++s) {
            if (tid < 64) {
                const int q = tid < LMS_ROW ? s_cov[s * LMS_ROW + tid] : -1;
                const unsigned long long b = __ballot(q >= 0 && s_rank[q >= 0 ? q : 0] == LMS_NONE);
                if (b == 0 ? tid == 0 : tid == __ffsll((long long)b) - 1) s_pick = b == 0 ? -1 : q;
            }
            __syncthreads();
            const int pick = s_pick;
            if (pick >= 0) {
                if (tid == 0) { s_rank[pick] = (uint16_t)n; s_list[n] = (uint16_t)pick; }
                ++n;
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        A.ref[f] = s_best ? 4095 - (s_best & 4095) : -1;
        A.n_voters[f] = voters;
        A.n_local[f] = n;
    }
    for (int k = tid; k < K; k += LMS_LANES) {
        A.local_kf[(size_t)f * K + k] = k < n ? (int)s_list[k] : -1;
        A.rank[(size_t)f * K + k] = s_rank[k];
    }
}

__global__ __launch_bounds__(LMS_LANES) void k_lms_points(LmsDev A)
{
    __shared__ uint16_t s_rank[YGZ_LMS_MAX_KEYFRAMES];
    __shared__ int32_t s_w[LMS_WAVES];
    const int tid = (int)threadIdx.x, f = (int)blockIdx.y, n_local = A.n_local[f];
    if ((int)blockIdx.x >= n_local) return;                                       // the whole workgroup
    lms_stage_rank(A, f, s_rank);
    for (int r = (int)blockIdx.x; r < n_local; r += (int)gridDim.x) {
        const int k = A.local_kf[(size_t)f * A.K + r];
        int c = 0, ft;
        for (int m = A.koff[k] + tid; m < A.koff[k + 1]; m += LMS_LANES) {
            const int p = A.kpt[m];
            c += A.pt_bad[p] == 0 && lms_first_rank(A, s_rank, p, &ft) == r;
        }
        c = ygz_wave_sum_i(c);
        if (ygz_lane() == 0) s_w[tid >> 6] = c;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < LMS_WAVES; ++w) t += s_w[w];
            A.cnt[(size_t)f * A.K + r] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(LMS_LANES) void k_lms_place(LmsDev A)
{
    __shared__ uint16_t s_rank[YGZ_LMS_MAX_KEYFRAMES];
    __shared__ int32_t s_start[YGZ_LMS_MAX_KEYFRAMES];
    __shared__ int32_t s_w[LMS_WAVES];
    const int tid = (int)threadIdx.x, lane = ygz_lane(), wave = tid >> 6, f = (int)blockIdx.y, n_local = A.n_local[f];
    // the scan of the frame's counts over the ranks, the same in every workgroup of the frame: a run of ranks per lane
    const int per = (n_local + LMS_LANES - 1) / LMS_LANES, r0 = min(tid * per, n_local), r1 = min(r0 + per, n_local);
    int sum = 0;
    for (int r = r0; r < r1; ++r) sum += A.cnt[(size_t)f * A.K + r];
    int incl = sum;
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int at = incl - sum, total = 0;
    for (int w = 0; w < LMS_WAVES; ++w) { const int c = s_w[w]; at += w < wave ? c : 0; total += c; }
    for (int r = r0; r < r1; ++r) { s_start[r] = at; at += A.cnt[(size_t)f * A.K + r]; }
    __syncthreads();
    if (blockIdx.x == 0) {
        const int kept = min(total, A.max_pt);
        for (int r = tid; r < n_local; r += LMS_LANES) A.start[(size_t)f * (A.K + 1) + r] = s_start[r];
        if (tid == 0) { A.start[(size_t)f * (A.K + 1) + n_local] = total; A.n_pt[f] = kept; A.n_cut[f] = total - kept; }
        for (int i = kept + tid; i < A.max_pt; i += LMS_LANES) A.local_pt[(size_t)f * A.max_pt + i] = -1;
    }
    if ((int)blockIdx.x >= n_local) return;                                       // the whole workgroup
    lms_stage_rank(A, f, s_rank);
    for (int r = (int)blockIdx.x; r < n_local; r += (int)gridDim.x) {
        const int base = s_start[r];
        if (base >= A.max_pt) break;                                              // the starts ascend: the rest is cut too
        const int k = A.local_kf[(size_t)f * A.K + r], m1 = A.koff[k + 1];
        int run = 0;
        for (int m0 = A.koff[k]; m0 < m1 && base + run < A.max_pt; m0 += LMS_LANES) {
            const int m = m0 + tid;
            int p = 0, ft = 0;
            bool keep = false;
            if (m < m1) {
                p = A.kpt[m];
                keep = A.pt_bad[p] == 0 && lms_first_rank(A, s_rank, p, &ft) == r;
            }
            int tot;
            const int pos = base + run + lms_block_rank(keep, s_w, &tot);
            if (keep && pos < A.max_pt) {
                A.local_pt[(size_t)f * A.max_pt + pos] = p;
                A.local_ft[(size_t)f * A.max_pt + pos] = ft;
            }
            run += tot;
        }
    }
}

__global__ __launch_bounds__(LMS_LANES) void k_lms_prior(LmsDev A)
{
    __shared__ uint16_t s_rank[YGZ_LMS_MAX_KEYFRAMES];
    const int f = (int)blockIdx.y, e = A.fr_off[f] + (int)blockIdx.x * LMS_LANES + (int)threadIdx.x, e1 = A.fr_off[f + 1];
    if (A.fr_off[f] + (int)blockIdx.x * LMS_LANES >= e1) return;                  // the whole workgroup
    lms_stage_rank(A, f, s_rank);
    if (e >= e1) return;
    const int p = A.fr_pt[e];
    int out = -1;
    if (p >= 0 && A.pt_bad[p] == 0) {
        int ft;
        const int r = lms_first_rank(A, s_rank, p, &ft);
        if (r != LMS_NONE) {
            const int32_t *start = A.start + (size_t)f * (A.K + 1), *pt = A.local_pt + (size_t)f * A.max_pt, *fts = A.local_ft + (size_t)f * A.max_pt;
            const int end = min(start[r + 1], A.max_pt);
            int lo = start[r], hi = end;
            for (int step = 0; step < 32 && lo < hi; ++step) {                    // the slice ascends by (feature, point)
                const int mid = lo + ((hi - lo) >> 1), mf = fts[mid];
                if (mf < ft || (mf == ft && pt[mid] < p)) lo = mid + 1;
                else hi = mid;
            }
            if (lo < end && pt[lo] == p) out = lo;
        }
    }
    A.fr_prior[e] = out;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
bool params_ok(const ygz_lms_params &q)
{
    return q.max_keyframes >= 1 && q.max_keyframes <= YGZ_LMS_MAX_KEYFRAMES && q.max_points >= 1;
}

}  // namespace

// the four launches on a bound table (lms_dev.h): what ygz_hip_local_map_select enqueues, and the resident call of rmap.hip on its own buffers
void ygz_lms_launch(ygz_hip_ctx *ctx, const LmsDev &A, int n_frames, int max_len)
{
    const int n_keyframes = A.K;
    const dim3 ranks((unsigned)std::min(n_keyframes, LMS_GRID_RANKS), (unsigned)n_frames);
    YGZ_LAUNCH(ctx, KID_LMS_VOTE, k_lms_vote, dim3((unsigned)n_frames), dim3(LMS_LANES), A);
    YGZ_LAUNCH(ctx, KID_LMS_POINTS, k_lms_points, ranks, dim3(LMS_LANES), A);
    YGZ_LAUNCH(ctx, KID_LMS_PLACE, k_lms_place, ranks, dim3(LMS_LANES), A);
    if (max_len > 0)
        YGZ_LAUNCH(ctx, KID_LMS_PRIOR, k_lms_prior, dim3((unsigned)ygz_div_up(max_len, LMS_LANES), (unsigned)n_frames), dim3(LMS_LANES), A);
}

extern "C" {

void ygz_hip_default_lms_params(ygz_lms_params *p)
{
    if (!p) return;
    p->max_keyframes = 80; p->max_points = 16384;
}

int ygz_hip_local_map_select(ygz_hip_ctx *ctx, int n_keyframes, const uint8_t *kf_bad, int n_cov, const int32_t *cov, int n_points,
                             const int32_t *offsets, const int32_t *kf, const int32_t *feat, const uint8_t *pt_bad, int n_frames,
                             const int32_t *fr_off, const int32_t *fr_pt, const ygz_lms_params *params, int32_t *votes, int32_t *ref,
                             int32_t *n_voters, int32_t *n_local, int32_t *local_kf, int32_t *n_pt, int32_t *n_cut, int32_t *local_pt,
                             int32_t *fr_prior)
{
    if (!kf_bad || !offsets || !kf || !feat || !fr_off || !fr_pt || !n_local || !local_kf || (n_cov > 0 && !cov)) return YGZ_E_INVALID;
    if (n_keyframes < 1 || n_cov < 0 || n_points < 1 || n_frames < 1) return YGZ_E_INVALID;
    if (n_keyframes > YGZ_LMS_MAX_KEYFRAMES || n_cov > YGZ_LMS_MAX_COV || n_frames > YGZ_LMS_MAX_FRAMES) return YGZ_E_CAPACITY;
    ygz_lms_params q;
    ygz_hip_default_lms_params(&q);
    if (params) q = *params;
    if (!params_ok(q)) return YGZ_E_INVALID;
    if ((int64_t)n_frames * q.max_points > YGZ_SLM_MAX_PAIRS || (int64_t)n_frames * n_keyframes > YGZ_COVIS_MAX_CELLS) return YGZ_E_CAPACITY;
    if (offsets[0] != 0 || fr_off[0] != 0) return YGZ_E_INVALID;
    bool big = false;
    for (int p = 0; p < n_points; ++p) {
        if (offsets[p + 1] < offsets[p]) return YGZ_E_INVALID;
        big = big || offsets[p + 1] - offsets[p] > YGZ_MAP_MAX_OBS_PER_POINT;
    }
    int max_len = 0;
    for (int f = 0; f < n_frames; ++f) {
        if (fr_off[f + 1] < fr_off[f]) return YGZ_E_INVALID;
        max_len = std::max(max_len, fr_off[f + 1] - fr_off[f]);
    }
    if (big || offsets[n_points] > YGZ_MAP_MAX_OBS || max_len > YGZ_LMS_MAX_FEATURES) return YGZ_E_CAPACITY;
    const int n_obs = offsets[n_points], n_ent = fr_off[n_frames];
    for (int p = 0; p < n_points; ++p)
        for (int g = offsets[p]; g < offsets[p + 1]; ++g)
            if (kf[g] < 0 || kf[g] >= n_keyframes || (g > offsets[p] && kf[g] <= kf[g - 1]) || feat[g] < 0 || feat[g] >= YGZ_LMS_FEAT_END)
                return YGZ_E_INVALID;
    for (size_t i = 0; i < (size_t)n_keyframes * (size_t)n_cov; ++i)
        if (cov[i] < -1 || cov[i] >= n_keyframes) return YGZ_E_INVALID;
    for (int e = 0; e < n_ent; ++e)
        if (fr_pt[e] < -1 || fr_pt[e] >= n_points) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    const size_t K = (size_t)n_keyframes, C = (size_t)n_cov, P = (size_t)n_points, N = (size_t)n_obs, F = (size_t)n_frames, E = (size_t)n_ent,
                 MP = (size_t)q.max_points;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    // [kf_bad | pt_bad | cov | offsets | obs | koff | kpt | fr_off | fr_pt) goes up, [ref .. fr_prior | votes) comes back (votes last: it is
    // left on the device when nobody asks for it), the rank table, the counts, their scan and the features of the kept points stay
    YgzBlobLayout L;
    const size_t o_kbad = L.add(K), o_pbad = L.add(P), o_cov = L.add_n<int32_t>(K * C), o_off = L.add_n<int32_t>(P + 1), o_obs = L.add_n<int32_t>(N);
    const size_t o_koff = L.add_n<int32_t>(K + 1), o_kpt = L.add_n<int32_t>(N), o_foff = L.add_n<int32_t>(F + 1), o_fpt = L.add_n<int32_t>(E);
    const size_t in_end = L.end;
    const size_t o_ref = L.add_n<int32_t>(F), o_nvot = L.add_n<int32_t>(F), o_nloc = L.add_n<int32_t>(F), o_npt = L.add_n<int32_t>(F);
    const size_t o_ncut = L.add_n<int32_t>(F), o_lkf = L.add_n<int32_t>(F * K), o_lpt = L.add_n<int32_t>(F * MP), o_prior = L.add_n<int32_t>(E);
    const size_t small_end = L.end, o_votes = L.add_n<int32_t>(F * K), out_end = L.end;
    const size_t o_rank = L.add_n<uint16_t>(F * K), o_cnt = L.add_n<int32_t>(F * K), o_start = L.add_n<int32_t>(F * (K + 1));
    const size_t o_lft = L.add_n<int32_t>(F * MP), total = L.end;
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_LMS, total, out_end, &b);
    if (rc != YGZ_OK) return rc;
    memcpy(b.host + o_kbad, kf_bad, K);
    if (pt_bad) memcpy(b.host + o_pbad, pt_bad, P);
    else memset(b.host + o_pbad, 0, P);
    if (C) memcpy(b.host + o_cov, cov, K * C * 4);
    memcpy(b.host + o_off, offsets, (P + 1) * 4);
    {
        int32_t *obs = ygz_at<int32_t>(b.host, o_obs);
        for (int g = 0; g < n_obs; ++g) obs[g] = kf[g] | (feat[g] << 16);
    }
    ygz_lms_build_index(n_points, offsets, kf, feat, n_keyframes, ygz_at<int32_t>(b.host, o_koff), ygz_at<int32_t>(b.host, o_kpt), nullptr);
    memcpy(b.host + o_foff, fr_off, (F + 1) * 4);
    if (E) memcpy(b.host + o_fpt, fr_pt, E * 4);
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    LmsDev A;
    A.K = n_keyframes; A.C = n_cov; A.max_kf = q.max_keyframes; A.max_pt = q.max_points;
    A.kf_bad = b.dev + o_kbad; A.pt_bad = b.dev + o_pbad;
    A.cov = ygz_at<const int32_t>(b.dev, o_cov); A.offsets = ygz_at<const int32_t>(b.dev, o_off); A.obs = ygz_at<const int32_t>(b.dev, o_obs);
    A.koff = ygz_at<const int32_t>(b.dev, o_koff); A.kpt = ygz_at<const int32_t>(b.dev, o_kpt);
    A.fr_off = ygz_at<const int32_t>(b.dev, o_foff); A.fr_pt = ygz_at<const int32_t>(b.dev, o_fpt);
    A.votes = ygz_at<int32_t>(b.dev, o_votes); A.ref = ygz_at<int32_t>(b.dev, o_ref); A.n_voters = ygz_at<int32_t>(b.dev, o_nvot);
    A.n_local = ygz_at<int32_t>(b.dev, o_nloc); A.local_kf = ygz_at<int32_t>(b.dev, o_lkf); A.n_pt = ygz_at<int32_t>(b.dev, o_npt);
    A.n_cut = ygz_at<int32_t>(b.dev, o_ncut); A.local_pt = ygz_at<int32_t>(b.dev, o_lpt); A.fr_prior = ygz_at<int32_t>(b.dev, o_prior);
    A.rank = ygz_at<uint16_t>(b.dev, o_rank); A.cnt = ygz_at<int32_t>(b.dev, o_cnt); A.start = ygz_at<int32_t>(b.dev, o_start);
    A.local_ft = ygz_at<int32_t>(b.dev, o_lft);
    ygz_lms_launch(ctx, A, n_frames, max_len);
    if ((rc = ygz_blob_fetch(ctx, b, o_ref, votes ? out_end : small_end)) != YGZ_OK) return rc;
    memcpy(n_local, b.host + o_nloc, F * 4);
    memcpy(local_kf, b.host + o_lkf, F * K * 4);
    if (votes) memcpy(votes, b.host + o_votes, F * K * 4);
    if (ref) memcpy(ref, b.host + o_ref, F * 4);
    if (n_voters) memcpy(n_voters, b.host + o_nvot, F * 4);
    if (n_pt) memcpy(n_pt, b.host + o_npt, F * 4);
    if (n_cut) memcpy(n_cut, b.host + o_ncut, F * 4);
    if (local_pt) memcpy(local_pt, b.host + o_lpt, F * MP * 4);
    if (fr_prior && E) memcpy(fr_prior, b.host + o_prior, E * 4);
    return YGZ_OK;
}

}  // extern "C"
