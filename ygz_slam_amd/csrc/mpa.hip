// Map-point attributes: ORB-SLAM2's MapPoint::UpdateNormalAndDepth as ygz::Matcher::PointAttributes states it (the mean viewing direction over
// the observations and dmax from the first one), for every point of a map in one call.  The map is a point-major CSR:
// point p owns the rows offsets[p] .. offsets[p + 1] - 1, a row names the observing keyframe and the pyramid level of the observation.
//
//   k_mpa_attr    lane = one point.  Consecutive lanes read consecutive runs of rows; the camera centres (at most 96 KiB) are read through L2.
//                 The sum over a point's rows is sequential in row order, in FP64 and uncontracted: every double is that of tests/mpa_ref.c,
//                 bit for bit.  A point without a row gets state 0, one with a distance of 0 or an output that is not finite state 2, and
//                 both get zeros: no NaN leaves the call.
//
// No atomic, no LDS, no wait for another workgroup, no scratch memory, no environment switch; the loop is a `for` over a count known at entry
// and every index a lane forms was validated by the entry point.  One packed upload, one launch, one copy back, one wait.
#include "ygz_internal.h"
#include "pose_block.h"
#include "mpa_dev.h"
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)

#define SCR_MPA 47                               // the packed block of ygz_hip_map_point_attributes: behind lms.hip's 46, the context's last
static_assert(SCR_MPA == YGZ_N_SCRATCH - 1, "47 is the last id ygz_hip_ctx::scratch holds: the next packed block needs a larger YGZ_N_SCRATCH");

namespace {

#define MPA_LANES 256

__global__ __launch_bounds__(MPA_LANES) void k_mpa_attr(MpaDev A)
{
    const int p = (int)blockIdx.x * MPA_LANES + (int)threadIdx.x;
    if (p >= A.P) return;
    const int a = A.offsets[p], b = A.offsets[p + 1];
    const double x = A.pw[3 * (size_t)p], y = A.pw[3 * (size_t)p + 1], z = A.pw[3 * (size_t)p + 2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, first = 0.0;
    bool zero = false;
    for (int e = a; e < b; ++e) {
        const double *c = A.center + 3 * (size_t)A.obs_kf[e];
        const double r0 = x - c[0], r1 = y - c[1], r2 = z - c[2];
        double q = r0 * r0;
        q = q + r1 * r1;
        q = q + r2 * r2;
        const double d = sqrt(q);
        zero = zero || d == 0.0;
        s0 += r0 / d; s1 += r1 / d; s2 += r2 / d;
        if (e == a) first = d;
    }
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, far = 0.0;
    int st = 0;
    if (b > a) {
        const int lv = max(A.obs_level[a], 0);
        const double cnt = (double)(b - a);
        n0 = s0 / cnt; n1 = s1 / cnt; n2 = s2 / cnt;
        far = first * (double)(1u << lv);                                         // lv <= 30: the power of two is exact
        st = (zero || !isfinite(far) || !isfinite(n0) || !isfinite(n1) || !isfinite(n2)) ? 2 : 1;
    }
    if (st != 1) { far = 0.0; n0 = 0.0; n1 = 0.0; n2 = 0.0; }
    A.dmax[p] = far;
    A.normal[3 * (size_t)p] = n0; A.normal[3 * (size_t)p + 1] = n1; A.normal[3 * (size_t)p + 2] = n2;
    A.state[p] = st;
}

}  // namespace

// the launch on a bound table (mpa_dev.h): ygz_hip_map_point_attributes on its packed block, rmap.hip on a resident map
void ygz_mpa_launch(ygz_hip_ctx *ctx, const MpaDev &A)
{
    YGZ_LAUNCH(ctx, KID_MPA_ATTR, k_mpa_attr, dim3((unsigned)ygz_div_up(A.P, MPA_LANES)), dim3(MPA_LANES), A);
}

extern "C" {

int ygz_hip_map_point_attributes(ygz_hip_ctx *ctx, int n_keyframes, const double *kf_center, int n_points, const double *pw,
                                 const int32_t *offsets, const int32_t *obs_kf, const int32_t *obs_level, double *dmax, double *normal,
                                 int32_t *state)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!kf_center || !pw || !offsets || !obs_kf || !obs_level || !dmax || !normal || !state || n_keyframes < 1 || n_points < 1)
        return YGZ_E_INVALID;
    if (n_keyframes > YGZ_MAP_MAX_KEYFRAMES || n_points > YGZ_MPA_MAX_POINTS) return YGZ_E_CAPACITY;
    if (offsets[0] != 0) return YGZ_E_INVALID;
    bool big = false;
    for (int p = 0; p < n_points; ++p) {
        if (offsets[p + 1] < offsets[p]) return YGZ_E_INVALID;
        big = big || offsets[p + 1] - offsets[p] > YGZ_MAP_MAX_OBS_PER_POINT;
    }
    if (big || offsets[n_points] > YGZ_MAP_MAX_OBS) return YGZ_E_CAPACITY;
    const int n_obs = offsets[n_points];
    for (int e = 0; e < n_obs; ++e)
        if (obs_kf[e] < 0 || obs_kf[e] >= n_keyframes || obs_level[e] > 30) return YGZ_E_INVALID;
    const size_t K = (size_t)n_keyframes, P = (size_t)n_points, N = (size_t)n_obs;
    if (!ygz_all_finite(kf_center, 3 * K) || !ygz_all_finite(pw, 3 * P)) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    // [centres | points | offsets | obs_kf | obs_level) goes up, [dmax | normal | state) comes back
    YgzBlobLayout L;
    const size_t o_c = L.add_n<double>(3 * K), o_pw = L.add_n<double>(3 * P), o_off = L.add_n<int32_t>(P + 1), o_kf = L.add_n<int32_t>(N);
    const size_t o_lv = L.add_n<int32_t>(N), in_end = L.end;
    const size_t o_dmax = L.add_n<double>(P), o_nrm = L.add_n<double>(3 * P), o_st = L.add_n<int32_t>(P), total = L.end;
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_MPA, total, total, &b);
    if (rc != YGZ_OK) return rc;
    memcpy(b.host + o_c, kf_center, 3 * K * 8);
    memcpy(b.host + o_pw, pw, 3 * P * 8);
    memcpy(b.host + o_off, offsets, (P + 1) * 4);
    if (N) { memcpy(b.host + o_kf, obs_kf, N * 4); memcpy(b.host + o_lv, obs_level, N * 4); }
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    MpaDev A;
    A.P = n_points;
    A.center = ygz_at<const double>(b.dev, o_c); A.pw = ygz_at<const double>(b.dev, o_pw);
    A.offsets = ygz_at<const int32_t>(b.dev, o_off); A.obs_kf = ygz_at<const int32_t>(b.dev, o_kf);
    A.obs_level = ygz_at<const int32_t>(b.dev, o_lv);
    A.dmax = ygz_at<double>(b.dev, o_dmax); A.normal = ygz_at<double>(b.dev, o_nrm); A.state = ygz_at<int32_t>(b.dev, o_st);
    ygz_mpa_launch(ctx, A);
    if ((rc = ygz_blob_fetch(ctx, b, o_dmax, total)) != YGZ_OK) return rc;
    memcpy(dmax, b.host + o_dmax, P * 8);
    memcpy(normal, b.host + o_nrm, 3 * P * 8);
    memcpy(state, b.host + o_st, P * 4);
    return YGZ_OK;
}

}  // extern "C"
