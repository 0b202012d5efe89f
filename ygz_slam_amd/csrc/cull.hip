// Keyframe culling: the redundancy counts of ORB-SLAM2's LocalMapping::KeyFrameCulling and its sequential walk.  The
// reference has the stage written and switched off (LocalMapping.cpp:579-618, its call at :327 commented out).  Both calls work on the
// point-major CSR of ygz_hip_covisibility plus the pyramid level of every observation; on the device an observation is ONE word,
// keyframe | level << 16.
//
//   k_cull_counts  every keyframe on the initial state.  A workgroup owns a contiguous run of CULL_RUN observations, lane = one observation
//                  (point p, keyframe a): it walks p's list, counts the other observers that pass the level test and adds 1 to tracked[a] and
//                  (count >= th_obs) to redundant[a] -- in LDS (2 x 4096 counters, 32 KiB), integer atomics.  The workgroup then adds its
//                  non-zero counters to the global ones.  Every point on one keyframe is 256 lanes on one LDS counter, never on one HBM word.
//   k_cull_walk    ONE resident workgroup of 1024 lanes steps through the candidates in the caller's order.  The host built the keyframe-major
//                  index of the candidates' observations; per candidate the lanes stride over its observations (any number of them), count as
//                  above with the removed flags (4096 bytes of LDS) and the dead flags of the state, and the sixteen wavefronts add their
//                  DPP sums to one of three rotating LDS slots.  After one barrier every lane forms the same decision
//                  (double)redundant > ratio * (double)tracked; on a cull the lanes stride again, take one `live` from each of the candidate's
//                  points and mark those that fall below min_obs, and a second barrier publishes it.  A keyframe holds a point once, so one
//                  lane owns one point of a cull: no atomics on the state.
//
// Integer sums and one double comparison: independent of the order the lanes arrive in.  No floating-point atomics, no wait for another
// workgroup, no scratch.  The arithmetic is that of tests/cull_ref.c, bit for bit.  Every index a kernel forms was validated by the entry point.
#include "ygz_internal.h"
#include <cmath>
#include <string.h>

namespace {

#define CULL_LANES      256                      // k_cull_counts
#define CULL_RUN        2048                     // observations of one workgroup of k_cull_counts
#define CULL_WALK_LANES 1024                     // k_cull_walk

// the observers of the point [a, b) other than entry g that are not removed and pass the level test
template <bool WITH_REMOVED>
__device__ __forceinline__ int cull_observers(const int32_t *__restrict__ kl, int a, int b, int g, int slack, const uint8_t *removed)
{
    const int top = slack < 0 ? 0x7FFF : (kl[g] >> 16) + slack;
    int n = 0;
    for (int j = a; j < b; ++j) {
        const int e = kl[j];
        bool ok = j != g && (e >> 16) <= top;
        if (WITH_REMOVED) ok = ok && removed[e & 0xFFFF] == 0;
        n += ok;
    }
    return n;
}

__global__ __launch_bounds__(CULL_LANES) void k_cull_counts(int n_obs, int K, const int32_t *__restrict__ offsets, const int32_t *__restrict__ owner,
                                                            const int32_t *__restrict__ kl, int th_obs, int slack, int32_t *__restrict__ counts)
{
    __shared__ int32_t s_cnt[2 * YGZ_CULL_MAX_KEYFRAMES];                         // [tracked K | redundant K]
    for (int i = (int)threadIdx.x; i < 2 * K; i += CULL_LANES) s_cnt[i] = 0;
    __syncthreads();
    const int first = (int)blockIdx.x * CULL_RUN, last = min(first + CULL_RUN, n_obs);
    for (int g = first + (int)threadIdx.x; g < last; g += CULL_LANES) {
        const int p = owner[g];
        const int n = cull_observers<false>(kl, offsets[p], offsets[p + 1], g, slack, nullptr);
        const int a = kl[g] & 0xFFFF;
        atomicAdd(&s_cnt[a], 1);
        if (n >= th_obs) atomicAdd(&s_cnt[K + a], 1);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < 2 * K; i += CULL_LANES) {
        const int v = s_cnt[i];
        if (v) atomicAdd(counts + i, v);
    }
}

__global__ __launch_bounds__(CULL_WALK_LANES) void k_cull_walk(int n_points, int K, int n_cand, const int32_t *__restrict__ offsets,
                                                               const int32_t *__restrict__ kl, const int32_t *__restrict__ cand,
                                                               const int32_t *__restrict__ koff, const int32_t *__restrict__ kobs,
                                                               const int32_t *__restrict__ kpt, int th_obs, int slack, int min_obs, double ratio,
                                                               int32_t *live, uint8_t *dead, int32_t *__restrict__ out)
{
    __shared__ uint8_t s_removed[YGZ_CULL_MAX_KEYFRAMES];
    __shared__ int32_t s_sum[3][2];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < K; i += CULL_WALK_LANES) s_removed[i] = 0;
    if (tid < 6) s_sum[tid >> 1][tid & 1] = 0;
    for (int p = tid; p < n_points; p += CULL_WALK_LANES) { live[p] = offsets[p + 1] - offsets[p]; dead[p] = 0; }
    __syncthreads();
    for (int i = 0; i < n_cand; ++i) {
        const int m0 = koff[i], m1 = koff[i + 1], slot = i % 3;
        int t = 0, r = 0;
        for (int m = m0 + tid; m < m1; m += CULL_WALK_LANES) {
            const int p = kpt[m];
            if (dead[p]) continue;
            ++t;
            r += cull_observers<true>(kl, offsets[p], offsets[p + 1], kobs[m], slack, s_removed) >= th_obs;
        }
        t = ygz_wave_sum_i(t);
        r = ygz_wave_sum_i(r);
        if (ygz_lane() == 0 && t) { atomicAdd(&s_sum[slot][0], t); atomicAdd(&s_sum[slot][1], r); }
        __syncthreads();
        const int tracked = s_sum[slot][0], redundant = s_sum[slot][1];
        const bool cull = (double)redundant > ratio * (double)tracked;
        if (tid == 0) {
            out[i] = cull; out[n_cand + i] = tracked; out[2 * n_cand + i] = redundant;
            // the slot of candidate i + 2: last read before this barrier, next written after the barrier of candidate i + 1
            const int z = (i + 2) % 3;
            s_sum[z][0] = 0; s_sum[z][1] = 0;
            if (cull) s_removed[cand[i]] = 1;
        }
        if (cull) {                                                               // the same in every lane
            for (int m = m0 + tid; m < m1; m += CULL_WALK_LANES) {
                const int p = kpt[m];
                const int l = live[p] - 1;
                live[p] = l;
                if (l < min_obs) dead[p] = 1;
            }
            __syncthreads();
        }
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
bool params_ok(const ygz_cull_params &q)
{
    return q.th_obs >= 1 && q.th_obs <= 256 && q.min_obs >= 0 && q.min_obs <= 256 && q.level_slack >= -1 && q.level_slack <= 15 &&
           std::isfinite(q.ratio) && q.ratio >= 0.0 && q.ratio <= 1.0;
}

// the checks both entry points share, in the header's order; *n_obs = offsets[n_points]
int check_lists(int n_points, const int32_t *offsets, const int32_t *kf, const int32_t *level, int K, int *n_obs)
{
    if (n_points < 1 || K < 1 || offsets[0] != 0) return YGZ_E_INVALID;
    bool big = false;
    for (int p = 0; p < n_points; ++p) {
        if (offsets[p + 1] < offsets[p]) return YGZ_E_INVALID;
        big = big || offsets[p + 1] - offsets[p] > YGZ_MAP_MAX_OBS_PER_POINT;
    }
    if (big || offsets[n_points] > YGZ_MAP_MAX_OBS) return YGZ_E_CAPACITY;
    for (int p = 0; p < n_points; ++p)
        for (int g = offsets[p]; g < offsets[p + 1]; ++g)
            if (kf[g] < 0 || kf[g] >= K || (g > offsets[p] && kf[g] <= kf[g - 1]) || level[g] < 0 || level[g] > 15) return YGZ_E_INVALID;
    *n_obs = offsets[n_points];
    return YGZ_OK;
}

void pack_lists(int n_obs, const int32_t *kf, const int32_t *level, int32_t *kl)
{
    for (int g = 0; g < n_obs; ++g) kl[g] = kf[g] | (level[g] << 16);
}

}  // namespace

extern "C" {

void ygz_hip_default_cull_params(ygz_cull_params *p)
{
    if (!p) return;
    p->th_obs = 3; p->level_slack = -1; p->min_obs = 2; p->pad = 0; p->ratio = 0.9;
}

int ygz_hip_keyframe_redundancy(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const int32_t *kf, const int32_t *level, int n_keyframes,
                                const ygz_cull_params *params, int32_t *tracked, int32_t *redundant)
{
    if (!offsets || !kf || !level || !tracked || !redundant) return YGZ_E_INVALID;
    if (n_keyframes > YGZ_CULL_MAX_KEYFRAMES) return YGZ_E_CAPACITY;
    ygz_cull_params q;
    ygz_hip_default_cull_params(&q);
    if (params) q = *params;
    if (!params_ok(q)) return YGZ_E_INVALID;
    int n_obs = 0;
    const int rv = check_lists(n_points, offsets, kf, level, n_keyframes, &n_obs);
    if (rv != YGZ_OK) return rv;
    if (!ctx) return YGZ_E_INVALID;
    const size_t P = (size_t)n_points, N = (size_t)n_obs, K = (size_t)n_keyframes;
    if (n_obs == 0) { memset(tracked, 0, K * 4); memset(redundant, 0, K * 4); return YGZ_OK; }
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    // [offsets | owner | kl) goes up, [counts) comes back
    YgzBlobLayout L;
    const size_t o_off = L.add_n<int32_t>(P + 1), o_own = L.add_n<int32_t>(N), o_kl = L.add_n<int32_t>(N), in_end = L.end;
    const size_t o_cnt = L.add_n<int32_t>(2 * K);
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_CULL, L.end, L.end, &b);
    if (rc != YGZ_OK) return rc;
    memcpy(b.host + o_off, offsets, (P + 1) * 4);
    int32_t *owner = ygz_at<int32_t>(b.host, o_own);
    for (int p = 0; p < n_points; ++p)
        for (int g = offsets[p]; g < offsets[p + 1]; ++g) owner[g] = p;
    pack_lists(n_obs, kf, level, ygz_at<int32_t>(b.host, o_kl));
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    YGZ_HIPCHK(ctx, hipMemsetAsync(b.dev + o_cnt, 0, 2 * K * 4, ctx->stream));
    YGZ_LAUNCH(ctx, KID_COUNT, k_cull_counts, dim3(ygz_div_up(n_obs, CULL_RUN)), dim3(CULL_LANES), n_obs, n_keyframes,
               ygz_at<const int32_t>(b.dev, o_off), ygz_at<const int32_t>(b.dev, o_own), ygz_at<const int32_t>(b.dev, o_kl), (int)q.th_obs,
               (int)q.level_slack, ygz_at<int32_t>(b.dev, o_cnt));
    if ((rc = ygz_blob_fetch(ctx, b, o_cnt, o_cnt + 2 * K * 4)) != YGZ_OK) return rc;
    memcpy(tracked, b.host + o_cnt, K * 4);
    memcpy(redundant, b.host + o_cnt + K * 4, K * 4);
    return YGZ_OK;
}

int ygz_hip_cull_keyframes(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const int32_t *kf, const int32_t *level, int n_keyframes,
                           int n_cand, const int32_t *cand, const ygz_cull_params *params, int32_t *culled, int32_t *tracked, int32_t *redundant,
                           uint8_t *point_dead)
{
    if (!offsets || !kf || !level || !cand || !culled || !tracked || !redundant) return YGZ_E_INVALID;
    if (n_keyframes > YGZ_CULL_MAX_KEYFRAMES || n_cand > YGZ_CULL_MAX_KEYFRAMES) return YGZ_E_CAPACITY;
    ygz_cull_params q;
    ygz_hip_default_cull_params(&q);
    if (params) q = *params;
    if (!params_ok(q) || n_cand < 1) return YGZ_E_INVALID;
    int n_obs = 0;
    const int rv = check_lists(n_points, offsets, kf, level, n_keyframes, &n_obs);
    if (rv != YGZ_OK) return rv;
    std::vector<int32_t> slot_of((size_t)n_keyframes, -1);
    for (int i = 0; i < n_cand; ++i) {
        if (cand[i] < 0 || cand[i] >= n_keyframes || slot_of[cand[i]] >= 0) return YGZ_E_INVALID;
        slot_of[cand[i]] = i;
    }
    if (!ctx) return YGZ_E_INVALID;
    const size_t P = (size_t)n_points, N = (size_t)n_obs, C = (size_t)n_cand;
    if (n_obs == 0) {
        memset(culled, 0, C * 4); memset(tracked, 0, C * 4); memset(redundant, 0, C * 4);
        if (point_dead) memset(point_dead, 0, P);
        return YGZ_OK;
    }
    // the keyframe-major index: the observations of candidate i are entries koff[i] .. koff[i + 1] - 1 of kobs (CSR row) / kpt (its point)
    std::vector<int32_t> koff(C + 1, 0);
    for (int g = 0; g < n_obs; ++g)
        if (slot_of[kf[g]] >= 0) ++koff[(size_t)slot_of[kf[g]] + 1];
    for (size_t i = 0; i < C; ++i) koff[i + 1] += koff[i];
    const size_t M = (size_t)koff[C];
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    // [offsets | kl | cand | koff | kobs | kpt) goes up, live stays, [out | dead) comes back
    YgzBlobLayout L;
    const size_t o_off = L.add_n<int32_t>(P + 1), o_kl = L.add_n<int32_t>(N), o_cand = L.add_n<int32_t>(C), o_koff = L.add_n<int32_t>(C + 1);
    const size_t o_kobs = L.add_n<int32_t>(M + 1), o_kpt = L.add_n<int32_t>(M + 1), in_end = L.end;
    const size_t o_live = L.add_n<int32_t>(P), o_out = L.add_n<int32_t>(3 * C), o_dead = L.add(P), total = L.end;
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_CULL, total, total, &b);
    if (rc != YGZ_OK) return rc;
    memcpy(b.host + o_off, offsets, (P + 1) * 4);
    pack_lists(n_obs, kf, level, ygz_at<int32_t>(b.host, o_kl));
    memcpy(b.host + o_cand, cand, C * 4);
    memcpy(b.host + o_koff, koff.data(), (C + 1) * 4);
    {
        int32_t *kobs = ygz_at<int32_t>(b.host, o_kobs), *kpt = ygz_at<int32_t>(b.host, o_kpt);
        std::vector<int32_t> fill(koff.begin(), koff.end() - 1);
        for (int p = 0; p < n_points; ++p)
            for (int g = offsets[p]; g < offsets[p + 1]; ++g) {
                const int s = slot_of[kf[g]];
                if (s < 0) continue;
                kobs[fill[s]] = g; kpt[fill[s]] = p; ++fill[s];
            }
    }
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    YGZ_LAUNCH(ctx, KID_COUNT, k_cull_walk, dim3(1), dim3(CULL_WALK_LANES), n_points, n_keyframes, n_cand, ygz_at<const int32_t>(b.dev, o_off),
               ygz_at<const int32_t>(b.dev, o_kl), ygz_at<const int32_t>(b.dev, o_cand), ygz_at<const int32_t>(b.dev, o_koff),
               ygz_at<const int32_t>(b.dev, o_kobs), ygz_at<const int32_t>(b.dev, o_kpt), (int)q.th_obs, (int)q.level_slack, (int)q.min_obs,
               q.ratio, ygz_at<int32_t>(b.dev, o_live), b.dev + o_dead, ygz_at<int32_t>(b.dev, o_out));
    if ((rc = ygz_blob_fetch(ctx, b, o_out, point_dead ? total : o_dead)) != YGZ_OK) return rc;
    memcpy(culled, b.host + o_out, C * 4);
    memcpy(tracked, b.host + o_out + C * 4, C * 4);
    memcpy(redundant, b.host + o_out + 2 * C * 4, C * 4);
    if (point_dead) memcpy(point_dead, b.host + o_dead, P);
    return YGZ_OK;
}

}  // extern "C"
