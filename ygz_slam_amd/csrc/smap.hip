// SM -- stereo map-point creation: ORB-SLAM2's two creation paths for a rectified rig.  Nothing in the reference, whose
// LocalMapping::CreateNewMapPoints (align.hip: ygz_hip_create_map_points) is monocular.  The frozen spec is tests/smap_ref.c (DESIGN.md section
// 24): uncontracted + - * / and sqrt in FP64, every sum in one stated order, no trigonometry; every output is bit-identical to it.
//   k_smap_pairs     lane = pair, over the concatenated pairs of all problems of the call, 64 lanes per workgroup.  A workgroup may straddle
//                    two problems: every lane looks its problem up in the offsets table (five halvings over at most 33 entries, the table in
//                    LDS) and reads that problem's two prepared cameras (rotation, translation, centre: 15 doubles each, prepared by the
//                    host in the restatement's order) through the caches.  Only the lanes that triangulate enter the 4 x 4 one-sided Jacobi,
//                    which lives in registers (all indices are compile-time constants after unrolling).
//   k_smap_keyframe  rank by (depth, index), selection and un-projection in one launch: every lane counts the features in front of its own over
//                    LDS tiles of 256 depths, and with them n_depth and the close ones, so no workgroup needs another's result.
// No atomic, no wait for another workgroup, no scratch, no environment switch.  init.hip's Jacobi is restated here, not shared.
#include "ygz_internal.h"
#include <math.h>
#include <string.h>
#include "pose_block.h"                 // ygz_all_finite
#pragma clang fp contract(off)

#define SM_PAIR_THREADS 64
#define SM_KF_THREADS   256
#define SM_CAM          15                  // doubles of a prepared camera: R (9, row-major), t (3), centre (3)
#define SM_DMAX 1.7976931348623157e308
#define SM_JACOBI_TOL 1e-15
#define SM_JACOBI_SWEEPS 40

struct SmapPairArgs {
    const int32_t *off;                     // [n_problems + 1]
    const double *cam;                      // [n_problems][2][SM_CAM]
    const double *px1, *px2, *ur1, *ur2, *depth1, *depth2;
    const int32_t *level1, *level2;
    int32_t *code, *method;
    double *pos;                            // [N][3]
    int n_problems, n_total;
    double K4[4];
    double baseline, bf, chi2_mono, chi2_stereo, cos_parallax_max, ratio_factor;
};

struct SmapKfArgs {
    const double *px, *depth;
    const uint8_t *has_point;
    int32_t *rank;
    uint8_t *selected;
    double *pos;
    int32_t *cnt;                           // n_depth, n_close
    int n, min_close;
    double th_depth;
    double K4[4];
    double cam[SM_CAM];
};

namespace {

// ---- the arithmetic (tests/smap_ref.c, function by function) ----------------------------------------------------------------------------
__device__ __forceinline__ double sm_cos_stereo(double d, double b)
{
    const double h = 0.5 * b, h2 = h * h, d2 = d * d;
    return (d2 - h2) / (d2 + h2);
}

__device__ __forceinline__ void sm_normalised(double u, double v, const double *K4, double *xn)
{
    xn[0] = (u - K4[2]) / K4[0]; xn[1] = (v - K4[3]) / K4[1]; xn[2] = 1.0;
}

__device__ __forceinline__ void sm_rt_mul(const double *R, const double *v, double *o)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (R[i] * v[0] + R[3 + i] * v[1]) + R[6 + i] * v[2];
}

__device__ __forceinline__ void sm_unproject(const double *C, const double *xn, double z, double *X)
{
    double c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = z * xn[i] - C[9 + i];
    sm_rt_mul(C, c, X);
}

__device__ __forceinline__ double sm_cam_row(const double *C, int r, const double *X)
{
    return ((C[3 * r] * X[0] + C[3 * r + 1] * X[1]) + C[3 * r + 2] * X[2]) + C[9 + r];
}

__device__ __forceinline__ bool sm_reproj_fails(const double *C, const double *X, double z, double pu, double pv, double ur, int level,
                                                const SmapPairArgs &A)
{
    const double x = sm_cam_row(C, 0, X), y = sm_cam_row(C, 1, X);
    const double u = A.K4[0] * (x / z) + A.K4[2], v = A.K4[1] * (y / z) + A.K4[3];
    const double ex = u - pu, ey = v - pv, s = (double)(1 << (2 * level));
    const double e2 = ex * ex + ey * ey;
    if (ur >= 0) {
        const double er = (u - A.bf / z) - ur;
        return e2 + er * er > A.chi2_stereo * s;
    }
    return e2 > A.chi2_mono * s;
}

__device__ __forceinline__ double sm_dist(const double *C, const double *X)
{
    const double a = X[0] - C[12], b = X[1] - C[13], c = X[2] - C[14];
    return sqrt((a * a + b * b) + c * c);
}

// ir_jacobi of tests/init_ref.c for a 4 x 4 system in registers: pair order (p, q), p < q, row by row; rotate when |gamma| > tol sqrt(alpha)
// sqrt(beta); at most 40 sweeps, a sweep without a rotation ends the loop
__device__ __forceinline__ void sm_jacobi4(double (&A)[16], double (&V)[16])
{
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < SM_JACOBI_SWEEPS; ++sweep) {
        int rotated = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double ap = A[i * 4 + p], aq = A[i * 4 + q];
                    alpha = alpha + ap * ap; beta = beta + aq * aq; gamma = gamma + ap * aq;
                }
                if (fabs(gamma) > SM_JACOBI_TOL * sqrt(alpha) * sqrt(beta)) {
                    rotated = 1;
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    double t;
                    if (fabs(zeta) > 1e150) t = 1.0 / (2.0 * zeta);
                    else t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double ap = A[i * 4 + p], aq = A[i * 4 + q];
                        A[i * 4 + p] = c * ap - s * aq;
                        A[i * 4 + q] = s * ap + c * aq;
                        const double vp = V[i * 4 + p], vq = V[i * 4 + q];
                        V[i * 4 + p] = c * vp - s * vq;
                        V[i * 4 + q] = s * vp + c * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
}

// ir_null_vector: the column of W = A V whose norm is <= every earlier one's, the last such
__device__ __forceinline__ void sm_null_vector4(double (&A)[16], double *x)
{
    double V[16];
    sm_jacobi4(A, V);
    int col = 0;
    double best = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double s = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double w = A[i * 4 + j]; s = s + w * w; }
        const double sv = sqrt(s);
        if (j == 0 || sv <= best) { col = j; best = sv; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = col == 0 ? V[k * 4] : (col == 1 ? V[k * 4 + 1] : (col == 2 ? V[k * 4 + 2] : V[k * 4 + 3]));
}

}  // namespace

__global__ __launch_bounds__(SM_PAIR_THREADS) void k_smap_pairs(SmapPairArgs A)
{
    __shared__ int32_t s_off[YGZ_SMAP_MAX_PROBLEMS + 1];
    const int tid = threadIdx.x;
    if (tid <= A.n_problems) s_off[tid] = A.off[tid];              // n_problems <= 32 < 64 lanes
    __syncthreads();
    const int i = (int)blockIdx.x * SM_PAIR_THREADS + tid;
    if (i >= A.n_total) return;
    // the problem of pair i: s_off[lo] <= i < s_off[hi] throughout, 32 entries halve to one in five steps (empty problems are skipped by it)
    int lo = 0, hi = A.n_problems;
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int mid = (lo + hi) >> 1;
        if (hi - lo > 1) { if (s_off[mid] <= i) lo = mid; else hi = mid; }
    }
    const double *C1 = A.cam + (size_t)lo * 2 * SM_CAM, *C2 = C1 + SM_CAM;
    const double u1 = A.px1[2 * (size_t)i], v1 = A.px1[2 * (size_t)i + 1], u2 = A.px2[2 * (size_t)i], v2 = A.px2[2 * (size_t)i + 1];
    const double ur1 = A.ur1[i], ur2 = A.ur2[i];
    const bool stereo1 = ur1 >= 0, stereo2 = ur2 >= 0;
    const double depth1 = stereo1 ? A.depth1[i] : 0.0, depth2 = stereo2 ? A.depth2[i] : 0.0;
    const int level1 = A.level1[i], level2 = A.level2[i];

    int code = 1, method = 0;
    double X[3] = { 0.0, 0.0, 0.0 }, out[3] = { 0.0, 0.0, 0.0 };
    double xn1[3], xn2[3], r1[3], r2[3];
    sm_normalised(u1, v1, A.K4, xn1); sm_normalised(u2, v2, A.K4, xn2);
    sm_rt_mul(C1, xn1, r1); sm_rt_mul(C2, xn2, r2);
    const double dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2];
    const double n1 = sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]), n2 = sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]);
    const double cosRays = dot / (n1 * n2);
    double cosS1 = cosRays + 1.0, cosS2 = cosRays + 1.0;
    if (stereo1) cosS1 = sm_cos_stereo(depth1, A.baseline);
    else if (stereo2) cosS2 = sm_cos_stereo(depth2, A.baseline);
    const double cosS = cosS1 < cosS2 ? cosS1 : cosS2;
    bool have = true;
    if (cosRays < cosS && cosRays > 0 && (stereo1 || stereo2 || cosRays < A.cos_parallax_max)) {
        method = 1;
        double M[16], x[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double a0 = c < 3 ? C1[c] : C1[9], a1 = c < 3 ? C1[3 + c] : C1[10], a2 = c < 3 ? C1[6 + c] : C1[11];
            const double b0 = c < 3 ? C2[c] : C2[9], b1 = c < 3 ? C2[3 + c] : C2[10], b2 = c < 3 ? C2[6 + c] : C2[11];
            M[0 * 4 + c] = xn1[0] * a2 - a0;
            M[1 * 4 + c] = xn1[1] * a2 - a1;
            M[2 * 4 + c] = xn2[0] * b2 - b0;
            M[3 * 4 + c] = xn2[1] * b2 - b1;
        }
        sm_null_vector4(M, x);
        if (x[3] == 0) { code = 2; have = false; }
        else {
#pragma unroll
            for (int k = 0; k < 3; ++k) X[k] = x[k] / x[3];
            if (!(fabs(X[0]) <= SM_DMAX && fabs(X[1]) <= SM_DMAX && fabs(X[2]) <= SM_DMAX)) { code = 2; have = false; }
        }
    } else if (stereo1 && cosS1 < cosS2) {
        method = 2;
        sm_unproject(C1, xn1, depth1, X);
    } else if (stereo2 && cosS2 < cosS1) {
        method = 3;
        sm_unproject(C2, xn2, depth2, X);
    } else have = false;
    if (have) {
        do {
            const double z1 = sm_cam_row(C1, 2, X);
            if (!(z1 > 0)) { code = 3; break; }
            const double z2 = sm_cam_row(C2, 2, X);
            if (!(z2 > 0)) { code = 4; break; }
            if (sm_reproj_fails(C1, X, z1, u1, v1, ur1, level1, A)) { code = 5; break; }
            if (sm_reproj_fails(C2, X, z2, u2, v2, ur2, level2, A)) { code = 6; break; }
            const double dist1 = sm_dist(C1, X), dist2 = sm_dist(C2, X);
            if (dist1 == 0 || dist2 == 0) { code = 7; break; }
            const double ratioDist = dist2 / dist1, ratioOctave = (double)(1 << level1) / (double)(1 << level2);
            if (ratioDist * A.ratio_factor < ratioOctave || ratioDist > ratioOctave * A.ratio_factor) { code = 8; break; }
            code = 0;
            out[0] = X[0]; out[1] = X[1]; out[2] = X[2];
        } while (false);
    }
    A.code[i] = code; A.method[i] = method;
    A.pos[3 * (size_t)i] = out[0]; A.pos[3 * (size_t)i + 1] = out[1]; A.pos[3 * (size_t)i + 2] = out[2];
}

__global__ __launch_bounds__(SM_KF_THREADS) void k_smap_keyframe(SmapKfArgs A)
{
    __shared__ double tile[SM_KF_THREADS];
    const int tid = threadIdx.x, i = (int)blockIdx.x * SM_KF_THREADS + tid, n = A.n;
    const double di = i < n ? A.depth[i] : 0.0, th = A.th_depth;
    int r = 0, nd = 0, c = 0;
    for (int base = 0; base < n; base += SM_KF_THREADS) {           // every lane of the workgroup walks every tile: the barriers are uniform
        const int j0 = base + tid;
        tile[tid] = j0 < n ? A.depth[j0] : 0.0;
        __syncthreads();
        // the whole tile, eight entries at a time and without a branch: the eight LDS reads (one address for all lanes: broadcasts) are in flight
        // together, and an entry past the end is 0.0 and counts nowhere
        for (int k0 = 0; k0 < SM_KF_THREADS; k0 += 8) {
            double d[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) d[u] = tile[k0 + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double dj = d[u];
                const int has = dj > 0 ? 1 : 0, before = (dj < di ? 1 : 0) | ((dj == di ? 1 : 0) & (base + k0 + u < i ? 1 : 0));
                nd += has;
                c += has & (dj <= th ? 1 : 0);
                r += has & before;
            }
        }
        __syncthreads();
    }
    if (i == 0) { A.cnt[0] = nd; A.cnt[1] = c; }
    if (i >= n) return;
    const int m = c > A.min_close ? c : A.min_close, last = nd - 1 < m ? nd - 1 : m;
    const bool walked = di > 0 && r <= last;
    const bool sel = walked && A.has_point[i] == 0;
    double X[3] = { 0.0, 0.0, 0.0 };
    if (sel) {
        double xn[3];
        sm_normalised(A.px[2 * (size_t)i], A.px[2 * (size_t)i + 1], A.K4, xn);
        sm_unproject(A.cam, xn, di, X);
    }
    A.rank[i] = walked ? r : -1;
    A.selected[i] = sel ? 1 : 0;
    A.pos[3 * (size_t)i] = X[0]; A.pos[3 * (size_t)i + 1] = X[1]; A.pos[3 * (size_t)i + 2] = X[2];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// sm_camera of the restatement: what a pose is prepared into, once per problem
static void smap_camera(const double *T, double *C)
{
    const double x = T[0], y = T[1], z = T[2], w = T[3];
    C[0] = 1.0 - 2.0 * (y * y + z * z); C[1] = 2.0 * (x * y - w * z);       C[2] = 2.0 * (x * z + w * y);
    C[3] = 2.0 * (x * y + w * z);       C[4] = 1.0 - 2.0 * (x * x + z * z); C[5] = 2.0 * (y * z - w * x);
    C[6] = 2.0 * (x * z - w * y);       C[7] = 2.0 * (y * z + w * x);       C[8] = 1.0 - 2.0 * (x * x + y * y);
    C[9] = T[4]; C[10] = T[5]; C[11] = T[6];
    for (int i = 0; i < 3; ++i) C[12 + i] = -((C[i] * C[9] + C[3 + i] * C[10]) + C[6 + i] * C[11]);
}

static bool smap_params_ok(const ygz_smap_params &p)
{
    if (!isfinite(p.baseline) || !isfinite(p.chi2_mono) || !isfinite(p.chi2_stereo) || !isfinite(p.cos_parallax_max) || !isfinite(p.ratio_factor) ||
        !isfinite(p.th_depth))
        return false;
    return p.baseline > 0.0 && p.chi2_mono > 0.0 && p.chi2_stereo > 0.0 && p.cos_parallax_max > 0.0 && p.th_depth > 0.0 && p.ratio_factor >= 1.0 &&
           p.min_close >= 0;
}

static bool smap_k_ok(const double *K4) { return ygz_all_finite(K4, 4) && K4[0] > 0.0 && K4[1] > 0.0; }

extern "C" {

void ygz_hip_default_smap_params(ygz_smap_params *p)
{
    if (!p) return;
    p->baseline = 0.1; p->chi2_mono = 5.991; p->chi2_stereo = 7.8; p->cos_parallax_max = 0.9998; p->ratio_factor = 3.0; p->th_depth = 3.5;
    p->min_close = 100; p->pad = 0;
}

int ygz_hip_stereo_create_map_points(ygz_hip_ctx *ctx, int n_problems, const ygz_smap_problem *problems, const double K4[4],
                                     const ygz_smap_params *params, int32_t *code, int32_t *method, double *pos_world, int32_t *counts)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!problems || !K4 || !code || !method || !pos_world || n_problems < 1) return YGZ_E_INVALID;
    if (n_problems > YGZ_SMAP_MAX_PROBLEMS) return YGZ_E_CAPACITY;
    size_t N = 0;
    for (int q = 0; q < n_problems; ++q) {
        if (problems[q].n < 0) return YGZ_E_INVALID;
        N += (size_t)problems[q].n;
    }
    if (N > YGZ_SMAP_MAX_PAIRS) return YGZ_E_CAPACITY;
    ygz_smap_params p;
    if (params) p = *params; else ygz_hip_default_smap_params(&p);
    if (!smap_params_ok(p) || !smap_k_ok(K4)) return YGZ_E_INVALID;
    for (int q = 0; q < n_problems; ++q) {
        const ygz_smap_problem &b = problems[q];
        if (!ygz_all_finite(b.T1, 7) || !ygz_all_finite(b.T2, 7)) return YGZ_E_INVALID;
        const size_t n = (size_t)b.n;
        if (!n) continue;
        if (!b.px1 || !b.px2 || !b.ur1 || !b.ur2 || !b.level1 || !b.level2) return YGZ_E_INVALID;
        if (!ygz_all_finite(b.px1, 2 * n) || !ygz_all_finite(b.px2, 2 * n) || !ygz_all_finite(b.ur1, n) || !ygz_all_finite(b.ur2, n)) return YGZ_E_INVALID;
        for (size_t i = 0; i < n; ++i) {
            if (b.ur1[i] >= 0 && (!b.depth1 || !isfinite(b.depth1[i]))) return YGZ_E_INVALID;
            if (b.ur2[i] >= 0 && (!b.depth2 || !isfinite(b.depth2[i]))) return YGZ_E_INVALID;
        }
    }
    if (!ctx) return YGZ_E_INVALID;
    for (int q = 0; q < n_problems; ++q)
        for (int i = 0; i < problems[q].n; ++i) {
            const int a = problems[q].level1[i], c = problems[q].level2[i];
            if (a < 0 || a >= ctx->prm.pyramid_levels || c < 0 || c >= ctx->prm.pyramid_levels) return YGZ_E_INVALID;
        }
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (counts) memset(counts, 0, (size_t)n_problems * 2 * sizeof(int32_t));
    if (N == 0) return YGZ_OK;                                      // nothing to create: no launch

    // up: [offsets | cameras | px1 | px2 | ur1 | ur2 | depth1 | depth2 | level1 | level2), back: [code | method | pos)
    const size_t P = (size_t)n_problems;
    YgzBlobLayout L;
    const size_t o_off = L.add_n<int32_t>(P + 1), o_cam = L.add_n<double>(P * 2 * SM_CAM);
    const size_t o_px1 = L.add_n<double>(N * 2), o_px2 = L.add_n<double>(N * 2), o_ur1 = L.add_n<double>(N), o_ur2 = L.add_n<double>(N);
    const size_t o_d1 = L.add_n<double>(N), o_d2 = L.add_n<double>(N), o_l1 = L.add_n<int32_t>(N), o_l2 = L.add_n<int32_t>(N), in_end = L.end;
    const size_t o_code = L.add_n<int32_t>(N), o_meth = L.add_n<int32_t>(N), o_pos = L.add_n<double>(N * 3), total = L.end;
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_SMAP, total, total, &b);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = b.host, *dev = b.dev;
    int32_t *off = ygz_at<int32_t>(up, o_off);
    size_t at = 0;
    for (int q = 0; q < n_problems; ++q) {
        const ygz_smap_problem &pb = problems[q];
        const size_t n = (size_t)pb.n;
        off[q] = (int32_t)at;
        smap_camera(pb.T1, ygz_at<double>(up, o_cam) + (size_t)q * 2 * SM_CAM);
        smap_camera(pb.T2, ygz_at<double>(up, o_cam) + (size_t)q * 2 * SM_CAM + SM_CAM);
        if (!n) continue;
        memcpy(ygz_at<double>(up, o_px1) + 2 * at, pb.px1, n * 16); memcpy(ygz_at<double>(up, o_px2) + 2 * at, pb.px2, n * 16);
        memcpy(ygz_at<double>(up, o_ur1) + at, pb.ur1, n * 8); memcpy(ygz_at<double>(up, o_ur2) + at, pb.ur2, n * 8);
        if (pb.depth1) memcpy(ygz_at<double>(up, o_d1) + at, pb.depth1, n * 8); else memset(ygz_at<double>(up, o_d1) + at, 0, n * 8);
        if (pb.depth2) memcpy(ygz_at<double>(up, o_d2) + at, pb.depth2, n * 8); else memset(ygz_at<double>(up, o_d2) + at, 0, n * 8);
        memcpy(ygz_at<int32_t>(up, o_l1) + at, pb.level1, n * 4); memcpy(ygz_at<int32_t>(up, o_l2) + at, pb.level2, n * 4);
        at += n;
    }
    off[n_problems] = (int32_t)at;
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;

    SmapPairArgs A;
    A.off = ygz_at<const int32_t>(dev, o_off); A.cam = ygz_at<const double>(dev, o_cam);
    A.px1 = ygz_at<const double>(dev, o_px1); A.px2 = ygz_at<const double>(dev, o_px2);
    A.ur1 = ygz_at<const double>(dev, o_ur1); A.ur2 = ygz_at<const double>(dev, o_ur2);
    A.depth1 = ygz_at<const double>(dev, o_d1); A.depth2 = ygz_at<const double>(dev, o_d2);
    A.level1 = ygz_at<const int32_t>(dev, o_l1); A.level2 = ygz_at<const int32_t>(dev, o_l2);
    A.code = ygz_at<int32_t>(dev, o_code); A.method = ygz_at<int32_t>(dev, o_meth); A.pos = ygz_at<double>(dev, o_pos);
    A.n_problems = n_problems; A.n_total = (int)N;
    for (int k = 0; k < 4; ++k) A.K4[k] = K4[k];
    A.baseline = p.baseline; A.bf = K4[0] * p.baseline; A.chi2_mono = p.chi2_mono; A.chi2_stereo = p.chi2_stereo;
    A.cos_parallax_max = p.cos_parallax_max; A.ratio_factor = p.ratio_factor;
    YGZ_LAUNCH(ctx, KID_SMAP_PAIRS, k_smap_pairs, dim3((unsigned)ygz_div_up((int)N, SM_PAIR_THREADS)), dim3(SM_PAIR_THREADS), A);
    if ((rc = ygz_blob_fetch(ctx, b, in_end, total)) != YGZ_OK) return rc;
    memcpy(code, up + o_code, N * 4); memcpy(method, up + o_meth, N * 4); memcpy(pos_world, up + o_pos, N * 24);
    if (counts)
        for (int q = 0; q < n_problems; ++q)
            for (int32_t i = off[q]; i < off[q + 1]; ++i)
                if (code[i] == 0) { ++counts[2 * q]; if (method[i] == 1) ++counts[2 * q + 1]; }
    return YGZ_OK;
}

int ygz_hip_stereo_keyframe_points(ygz_hip_ctx *ctx, const double T[7], int n, const double *px, const double *depth, const uint8_t *has_point,
                                   const double K4[4], const ygz_smap_params *params, int32_t *rank, uint8_t *selected, double *pos_world,
                                   int *n_depth, int *n_close, int *n_selected)
{
    if (!T || !K4 || n < 0) return YGZ_E_INVALID;
    if (n > 0 && (!px || !depth || !has_point || !rank || !selected || !pos_world)) return YGZ_E_INVALID;
    ygz_smap_params p;
    if (params) p = *params; else ygz_hip_default_smap_params(&p);
    if (!smap_params_ok(p) || !smap_k_ok(K4) || !ygz_all_finite(T, 7)) return YGZ_E_INVALID;
    if (n > 0 && (!ygz_all_finite(px, 2 * (size_t)n) || !ygz_all_finite(depth, (size_t)n))) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    if (n > ctx->cells) return YGZ_E_CAPACITY;
    YgzDeviceGuard dg_(ctx);
    { int rj = ygz_join(ctx); if (rj != YGZ_OK) return rj; }
    if (n_depth) *n_depth = 0;
    if (n_close) *n_close = 0;
    if (n_selected) *n_selected = 0;
    if (n == 0) return YGZ_OK;

    const size_t N = (size_t)n;
    YgzBlobLayout L;
    const size_t o_px = L.add_n<double>(N * 2), o_dp = L.add_n<double>(N), o_has = L.add_n<uint8_t>(N), in_end = L.end;
    const size_t o_rank = L.add_n<int32_t>(N), o_sel = L.add_n<uint8_t>(N), o_pos = L.add_n<double>(N * 3), o_cnt = L.add_n<int32_t>(2), total = L.end;
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_SMAP, total, total, &b);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = b.host, *dev = b.dev;
    memcpy(up + o_px, px, N * 16); memcpy(up + o_dp, depth, N * 8); memcpy(up + o_has, has_point, N);
    if ((rc = ygz_blob_upload(ctx, b, in_end)) != YGZ_OK) return rc;
    SmapKfArgs A;
    A.px = ygz_at<const double>(dev, o_px); A.depth = ygz_at<const double>(dev, o_dp); A.has_point = ygz_at<const uint8_t>(dev, o_has);
    A.rank = ygz_at<int32_t>(dev, o_rank); A.selected = ygz_at<uint8_t>(dev, o_sel); A.pos = ygz_at<double>(dev, o_pos);
    A.cnt = ygz_at<int32_t>(dev, o_cnt);
    A.n = n; A.min_close = p.min_close; A.th_depth = p.th_depth;
    for (int k = 0; k < 4; ++k) A.K4[k] = K4[k];
    smap_camera(T, A.cam);
    YGZ_LAUNCH(ctx, KID_SMAP_KEYFRAME, k_smap_keyframe, dim3((unsigned)ygz_div_up(n, SM_KF_THREADS)), dim3(SM_KF_THREADS), A);
    if ((rc = ygz_blob_fetch(ctx, b, in_end, total)) != YGZ_OK) return rc;
    memcpy(rank, up + o_rank, N * 4); memcpy(selected, up + o_sel, N); memcpy(pos_world, up + o_pos, N * 24);
    const int32_t *cnt = ygz_at<const int32_t>(up, o_cnt);
    if (n_depth) *n_depth = cnt[0];
    if (n_close) *n_close = cnt[1];
    if (n_selected) { int s = 0; for (size_t i = 0; i < N; ++i) s += selected[i] ? 1 : 0; *n_selected = s; }
    return YGZ_OK;
}

}  // extern "C"
