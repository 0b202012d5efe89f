// Map upkeep after a loop correction: the two batch integer jobs that fusing duplicated map points forces.  Nothing in
// the reference: MapPoint::ComputeDistinctiveDesc is shipped commented out and the covisibility weights exist only as a std::map walk per
// keyframe.  Both work on a CSR of observations: point p owns rows offsets[p] .. offsets[p+1]-1.
//
//   k_map_median   lane = one observation.  It keeps its 256-bit descriptor in eight registers and walks its point's range; the median of its
//                  distance row (element (n-1)/2 of the ascending row, the self distance included) is the smallest v in [0, 256] with
//                  count(d <= v) >= (n-1)/2 + 1, found by a nine-step descent over v that recomputes the distances (eight popcounts each):
//                  no sorted row, no per-lane array, no scratch.  atomicMin on the point's key (median << 16 | observation) gives ORB-SLAM2's
//                  "smallest median, first of equals".  The lanes of a point read the same descriptor at the same time: one fetch per wave.
//   k_map_covis    lane = one observation (point p, keyframe a).  When a is a row it walks p's list and adds 1 to weights[row(a)][b] for
//                  every b, b = a included: the diagonal counts the points that hold the row.
//
// Both results are sums / minima of integers: independent of the order the lanes arrive in.  One upload from page-locked memory (the keys'
// initial value travels with it), the launches, one copy back, one wait.  The arithmetic is that of tests/map_ref.c, bit for bit.
#include "ygz_internal.h"
#include <string.h>

namespace {

#define MAP_LANES 256

__global__ __launch_bounds__(MAP_LANES) void k_map_median(int n_obs, const int32_t *__restrict__ offsets, const int32_t *__restrict__ owner,
                                                          const uint32_t *__restrict__ desc, uint32_t *__restrict__ keys)
{
    const int g = blockIdx.x * MAP_LANES + threadIdx.x;
    if (g >= n_obs) return;
    const int p = owner[g];
    const int a = offsets[p], b = offsets[p + 1];
    const uint4 lo = *reinterpret_cast<const uint4 *>(desc + 8 * (size_t)g), hi = *reinterpret_cast<const uint4 *>(desc + 8 * (size_t)g + 4);
    const int need = (b - a - 1) / 2 + 1;
    // the largest v with count(d <= v - 1) < need = the smallest v with count(d <= v) >= need
    int v = 0;
    for (int step = 256; step >= 1; step >>= 1) {
        const int t = v + step - 1;
        int c = 0;
        for (int j = a; j < b; ++j) {
            const uint4 x = *reinterpret_cast<const uint4 *>(desc + 8 * (size_t)j), y = *reinterpret_cast<const uint4 *>(desc + 8 * (size_t)j + 4);
            const int d = __popc(lo.x ^ x.x) + __popc(lo.y ^ x.y) + __popc(lo.z ^ x.z) + __popc(lo.w ^ x.w) +
                          __popc(hi.x ^ y.x) + __popc(hi.y ^ y.y) + __popc(hi.z ^ y.z) + __popc(hi.w ^ y.w);
            c += d <= t;
        }
        if (c < need) v += step;
    }
    atomicMin(keys + p, ((uint32_t)v << 16) | (uint32_t)(g - a));
}

__global__ __launch_bounds__(MAP_LANES) void k_map_covis(int n_obs, int K, const int32_t *__restrict__ offsets, const int32_t *__restrict__ owner,
                                                         const int32_t *__restrict__ kf, const int32_t *__restrict__ row_of,
                                                         int32_t *__restrict__ weights)
{
    const int g = blockIdx.x * MAP_LANES + threadIdx.x;
    if (g >= n_obs) return;
    const int r = row_of[kf[g]];
    if (r < 0) return;
    const int p = owner[g];
    const int a = offsets[p], b = offsets[p + 1];
    int32_t *w = weights + (size_t)r * (size_t)K;
    for (int j = a; j < b; ++j) atomicAdd(w + kf[j], 1);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// offsets [n_points + 1]: starts at 0, never decreases; *n_obs = its last entry.  per_point > 0: no point holds more
int check_offsets(int n_points, const int32_t *offsets, int per_point, int *n_obs)
{
    if (n_points < 1 || offsets[0] != 0) return YGZ_E_INVALID;
    bool big = false;
    for (int p = 0; p < n_points; ++p) {
        if (offsets[p + 1] < offsets[p]) return YGZ_E_INVALID;
        big = big || (per_point > 0 && offsets[p + 1] - offsets[p] > per_point);
    }
    if (big || offsets[n_points] > YGZ_MAP_MAX_OBS) return YGZ_E_CAPACITY;
    *n_obs = offsets[n_points];
    return YGZ_OK;
}

void fill_owner(int n_points, const int32_t *offsets, int32_t *owner)
{
    for (int p = 0; p < n_points; ++p)
        for (int g = offsets[p]; g < offsets[p + 1]; ++g) owner[g] = p;
}

}  // namespace

extern "C" {

int ygz_hip_distinctive_descriptors(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const uint8_t *desc, int32_t *best, int32_t *median,
                                    uint8_t *out_desc)
{
    if (!offsets || !desc || !best) return YGZ_E_INVALID;
    int n_obs = 0;
    const int rv = check_offsets(n_points, offsets, YGZ_MAP_MAX_OBS_PER_POINT, &n_obs);
    if (rv != YGZ_OK) return rv;
    if (!ctx) return YGZ_E_INVALID;
    const size_t P = (size_t)n_points, N = (size_t)n_obs;
    const uint32_t *keys = nullptr;
    if (n_obs > 0) {
        YgzDeviceGuard dg_(ctx);
        { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
        // [offsets | owner | desc | keys) goes up, [keys) comes back
        YgzBlobLayout L;
        const size_t o_off = L.add_n<int32_t>(P + 1), o_own = L.add_n<int32_t>(N), o_desc = L.add_n<uint32_t>(N * 8), o_keys = L.add_n<uint32_t>(P);
        YgzBlob b;
        int rc = ygz_blob_open(ctx, SCR_MAP, L.end, L.end, &b);
        if (rc != YGZ_OK) return rc;
        memcpy(b.host + o_off, offsets, (P + 1) * 4);
        fill_owner(n_points, offsets, ygz_at<int32_t>(b.host, o_own));
        memcpy(b.host + o_desc, desc, N * 32);
        memset(b.host + o_keys, 0xFF, P * 4);
        if ((rc = ygz_blob_upload(ctx, b, L.end)) != YGZ_OK) return rc;
        YGZ_LAUNCH(ctx, KID_COUNT, k_map_median, dim3(ygz_div_up(n_obs, MAP_LANES)), dim3(MAP_LANES), n_obs, ygz_at<const int32_t>(b.dev, o_off),
                   ygz_at<const int32_t>(b.dev, o_own), ygz_at<const uint32_t>(b.dev, o_desc), ygz_at<uint32_t>(b.dev, o_keys));
        if ((rc = ygz_blob_fetch(ctx, b, o_keys, o_keys + P * 4)) != YGZ_OK) return rc;
        keys = ygz_at<const uint32_t>(b.host, o_keys);
    }
    // the key names the observation; its 32 bytes are the caller's own
    for (int p = 0; p < n_points; ++p) {
        const bool any = keys && offsets[p + 1] > offsets[p];
        const int i = any ? (int)(keys[p] & 0xFFFFu) : -1;
        best[p] = i;
        if (median) median[p] = any ? (int32_t)(keys[p] >> 16) : -1;
        if (!out_desc) continue;
        if (any) memcpy(out_desc + 32 * (size_t)p, desc + 32 * ((size_t)offsets[p] + (size_t)i), 32);
        else memset(out_desc + 32 * (size_t)p, 0, 32);
    }
    return YGZ_OK;
}

int ygz_hip_covisibility(ygz_hip_ctx *ctx, int n_points, const int32_t *offsets, const int32_t *kf, int n_keyframes, int n_rows,
                         const int32_t *rows, int32_t *weights)
{
    if (!offsets || !kf || !rows || !weights) return YGZ_E_INVALID;
    if (n_keyframes > YGZ_MAP_MAX_KEYFRAMES) return YGZ_E_CAPACITY;
    if (n_keyframes < 1 || n_rows < 1) return YGZ_E_INVALID;
    if ((long long)n_rows * (long long)n_keyframes > (long long)YGZ_COVIS_MAX_CELLS) return YGZ_E_CAPACITY;
    int n_obs = 0;
    const int rv = check_offsets(n_points, offsets, 0, &n_obs);
    if (rv != YGZ_OK) return rv;
    for (int p = 0; p < n_points; ++p)
        for (int g = offsets[p]; g < offsets[p + 1]; ++g)
            if (kf[g] < 0 || kf[g] >= n_keyframes || (g > offsets[p] && kf[g] <= kf[g - 1])) return YGZ_E_INVALID;
    std::vector<int32_t> row_of((size_t)n_keyframes, -1);
    for (int r = 0; r < n_rows; ++r) {
        if (rows[r] < 0 || rows[r] >= n_keyframes || row_of[rows[r]] >= 0) return YGZ_E_INVALID;
        row_of[rows[r]] = r;
    }
    if (!ctx) return YGZ_E_INVALID;
    const size_t P = (size_t)n_points, N = (size_t)n_obs, K = (size_t)n_keyframes, W = (size_t)n_rows * K * 4;
    if (n_obs == 0) { memset(weights, 0, W); return YGZ_OK; }
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    // [offsets | owner | kf | row_of) goes up, [weights) comes back
    YgzBlobLayout L;
    const size_t o_off = L.add_n<int32_t>(P + 1), o_own = L.add_n<int32_t>(N), o_kf = L.add_n<int32_t>(N), o_row = L.add_n<int32_t>(K), in_end = L.end;
    const size_t o_w = L.add(W);
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_MAP, L.end, L.end, &b);
    if (rc != YGZ_OK) return rc;
    memcpy(b.host + o_off, offsets, (P + 1) * 4);
    fill_owner(n_points, offsets, ygz_at<int32_t>(b.host, o_own));
    memcpy(b.host + o_kf, kf, N * 4);
    memcpy(b.host + o_row, row_of.data(), K * 4);
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    YGZ_HIPCHK(ctx, hipMemsetAsync(b.dev + o_w, 0, W, ctx->stream));
    YGZ_LAUNCH(ctx, KID_COUNT, k_map_covis, dim3(ygz_div_up(n_obs, MAP_LANES)), dim3(MAP_LANES), n_obs, n_keyframes,
               ygz_at<const int32_t>(b.dev, o_off), ygz_at<const int32_t>(b.dev, o_own), ygz_at<const int32_t>(b.dev, o_kf),
               ygz_at<const int32_t>(b.dev, o_row), ygz_at<int32_t>(b.dev, o_w));
    if ((rc = ygz_blob_fetch(ctx, b, o_w, o_w + W)) != YGZ_OK) return rc;
    memcpy(weights, b.host + o_w, W);
    return YGZ_OK;
}

}  // extern "C"
