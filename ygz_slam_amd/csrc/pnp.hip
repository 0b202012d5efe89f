// Relocalisation pose -- P3P RANSAC over several independent 2D-3D problems (one per candidate keyframe).  Nothing in the reference: it
// fills the stub at src/Module/VisualOdometry.cpp:101-104 ("try relocalization"), as ORB-SLAM2's Tracking::Relocalization does.  The
// arithmetic is tests/pnp_ref.c's decision by decision (-ffp-contract=off, only + - * / and sqrt), so every output is bit-identical to it
// (DESIGN.md section 10).  One call = one upload, three launches on the context's stream, one copy back, one wait:
//   k_pnp_solve    lane = (problem, sample): Lambda Twist P3P of the sample's three correspondences, up to 4 poses
//   k_pnp_score    lane = (problem, hypothesis = sample * 4 + solution), the problem's points staged in LDS: the inlier count
//   k_pnp_select   block = problem: the highest count (ties: smallest hypothesis), R, t, T_cw, the inlier mask
// PnpIn, PnpDev and the kernels' prototypes are in pnp_dev.h: srl.hip launches the same three kernels on associations it compacted itself.
#include "ygz_internal.h"
#include "pnp_dev.h"
#include "posemath_dev.h"
#include <cstring>

using namespace ygz_pnp;

namespace {

// ---- the arithmetic (tests/pnp_ref.c, function by function; 3 x 3 inverse and matrix -> quaternion: posemath_dev.h) -----------------
#define PR_BISECT 64
#define PR_REFINE 5

__device__ __forceinline__ int root2real(double b, double c, double *r1, double *r2)
{
    const double v = b * b - 4.0 * c;
    if (!(v >= 0)) { *r1 = 0; *r2 = 0; return 0; }
    const double y = sqrt(v);
    if (b < 0) { *r1 = 0.5 * (-b + y); *r2 = 2.0 * c / (-b + y); }
    else if (b > 0) { *r1 = 2.0 * c / (-b - y); *r2 = 0.5 * (-b - y); }
    else { *r1 = 0.5 * y; *r2 = -0.5 * y; }
    return 1;
}

__device__ __forceinline__ double cubic_at(double x, double b, double c, double d) { return ((x + b) * x + c) * x + d; }

// the largest real root of x^3 + b x^2 + c x + d: a bracket on which the cubic is monotone, then PR_BISECT halvings
__device__ __forceinline__ double pr_cubic_root(double b, double c, double d)
{
    double B = fabs(b);
    if (fabs(c) > B) B = fabs(c);
    if (fabs(d) > B) B = fabs(d);
    B = B + 1.0;
    double lo = -B, hi = B;
    const double disc = b * b - 3.0 * c;
    if (disc > 0) {
        const double sq = sqrt(disc);
        const double x1 = (-b - sq) / 3.0, x2 = (-b + sq) / 3.0;
        if (cubic_at(x2, b, c, d) <= 0) lo = x2;
        else hi = x1;
    }
    for (int k = 0; k < PR_BISECT; ++k) {
        const double m = 0.5 * (lo + hi);
        if (cubic_at(m, b, c, d) <= 0) lo = m;
        else hi = m;
    }
    return 0.5 * (lo + hi);
}

// the eigenvectors of the two non-zero eigenvalues of the symmetric A (one eigenvalue is 0), larger |eigenvalue| first
__device__ __forceinline__ void pr_eig_known0(const double *A, double *V, double *L)
{
    const double b = -A[0] - A[4] - A[8];
    const double c = -A[1] * A[1] - A[2] * A[2] - A[5] * A[5] + A[0] * (A[4] + A[8]) + A[4] * A[8];
    double e1, e2;
    root2real(b, c, &e1, &e2);
    if (fabs(e1) < fabs(e2)) { const double t = e1; e1 = e2; e2 = t; }
    L[0] = e1; L[1] = e2;
    const double mx0 = A[1] * A[5] - A[2] * A[4];
    const double mx1 = A[1] * A[2] - A[0] * A[5];
    const double mx2 = A[0] * A[4] - A[1] * A[1];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double e = k == 0 ? e1 : e2;
        const double tmp = 1.0 / (e * e - e * (A[0] + A[4]) + mx2);
        const double a1 = (e * A[2] + mx0) * tmp;
        const double a2 = (e * A[5] + mx1) * tmp;
        const double rn = 1.0 / sqrt(a1 * a1 + a2 * a2 + 1.0);
        V[3 * k + 0] = a1 * rn; V[3 * k + 1] = a2 * rn; V[3 * k + 2] = rn;
    }
}

__device__ __forceinline__ double residual_l1(const double *l, double a12, double a13, double a23, double b12, double b13, double b23, double *r)
{
    r[0] = l[0] * l[0] + l[1] * l[1] + b12 * l[0] * l[1] - a12;
    r[1] = l[0] * l[0] + l[2] * l[2] + b13 * l[0] * l[2] - a13;
    r[2] = l[1] * l[1] + l[2] * l[2] + b23 * l[1] * l[2] - a23;
    return fabs(r[0]) + fabs(r[1]) + fabs(r[2]);
}

__device__ __forceinline__ void pr_refine(double *l, double a12, double a13, double a23, double b12, double b13, double b23)
{
    for (int it = 0; it < PR_REFINE; ++it) {
        double r[3], rn[3], ln[3];
        const double e = residual_l1(l, a12, a13, a23, b12, b13, b23, r);
        const double j11 = 2.0 * l[0] + b12 * l[1], j12 = 2.0 * l[1] + b12 * l[0];
        const double j21 = 2.0 * l[0] + b13 * l[2], j23 = 2.0 * l[2] + b13 * l[0];
        const double j32 = 2.0 * l[1] + b23 * l[2], j33 = 2.0 * l[2] + b23 * l[1];
        const double det = -j11 * j23 * j32 - j12 * j21 * j33;
        if (!(fabs(det) > 0)) break;
        const double d1 = (-j23 * j32 * r[0] - j12 * j33 * r[1] + j12 * j23 * r[2]) / det;
        const double d2 = (-j21 * j33 * r[0] + j11 * j33 * r[1] - j11 * j23 * r[2]) / det;
        const double d3 = (j21 * j32 * r[0] - j11 * j32 * r[1] - j12 * j21 * r[2]) / det;
        ln[0] = l[0] - d1; ln[1] = l[1] - d2; ln[2] = l[2] - d3;
        if (!(residual_l1(ln, a12, a13, a23, b12, b13, b23, rn) < e)) break;
        l[0] = ln[0]; l[1] = ln[1]; l[2] = ln[2];
    }
}

__device__ __forceinline__ void bearing(const double *px, const double *K4, double *y)
{
    const double x = (px[0] - K4[2]) / K4[0], v = (px[1] - K4[3]) / K4[1];
    const double n = sqrt(x * x + v * v + 1.0);
    y[0] = x / n; y[1] = v / n; y[2] = 1.0 / n;
}

__device__ __forceinline__ int pose_from_depths(const double *l, const double *y1, const double *y2, const double *y3, const double *x1,
                                                const double *Xi, double *out)
{
    double r1[3], yd1[3], yd2[3], Y[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r1[k] = y1[k] * l[0];
        yd1[k] = r1[k] - y2[k] * l[1];
        yd2[k] = r1[k] - y3[k] * l[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { Y[k * 3 + 0] = yd1[k]; Y[k * 3 + 1] = yd2[k]; }
    Y[2] = yd1[1] * yd2[2] - yd1[2] * yd2[1];
    Y[5] = yd1[2] * yd2[0] - yd1[0] * yd2[2];
    Y[8] = yd1[0] * yd2[1] - yd1[1] * yd2[0];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = Y[i * 3 + 0] * Xi[0 * 3 + j] + Y[i * 3 + 1] * Xi[1 * 3 + j] + Y[i * 3 + 2] * Xi[2 * 3 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[9 + i] = r1[i] - (out[i * 3 + 0] * x1[0] + out[i * 3 + 1] * x1[1] + out[i * 3 + 2] * x1[2]);
    int ok = 1;
#pragma unroll
    for (int k = 0; k < 12; ++k) ok &= fabs(out[k]) <= 1e300;
    return ok;
}

// pr_p3p: the poses go straight to the lane's 4 x 12 slots in global memory (a run-time slot index into a register array would put it in
// scratch memory); the candidate loops are unrolled, so every local array below has constant indices only
__device__ __forceinline__ int pr_p3p(const double *pw, const double *px, const double *K4, double *sol)
{
    const double *x1 = pw, *x2 = pw + 3, *x3 = pw + 6;
    double d12[3], d13[3], d23[3], nx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d12[k] = x1[k] - x2[k]; d13[k] = x1[k] - x3[k]; d23[k] = x2[k] - x3[k]; }
    nx[0] = d12[1] * d13[2] - d12[2] * d13[1];
    nx[1] = d12[2] * d13[0] - d12[0] * d13[2];
    nx[2] = d12[0] * d13[1] - d12[1] * d13[0];
    const double a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double a23 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
    const double nn = nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2];
    if (!(nn > 1e-10 * a12 * a13)) return 0;
    double y1[3], y2[3], y3[3];
    bearing(px, K4, y1); bearing(px + 2, K4, y2); bearing(px + 4, K4, y3);
    const double b12 = -2.0 * (y1[0] * y2[0] + y1[1] * y2[1] + y1[2] * y2[2]);
    const double b13 = -2.0 * (y1[0] * y3[0] + y1[1] * y3[1] + y1[2] * y3[2]);
    const double b23 = -2.0 * (y2[0] * y3[0] + y2[1] * y3[1] + y2[2] * y3[2]);
    const double c31 = -0.5 * b13, c23 = -0.5 * b23, c12 = -0.5 * b12;
    const double blob = c12 * c23 * c31 - 1.0;
    const double s31 = 1.0 - c31 * c31, s23 = 1.0 - c23 * c23, s12 = 1.0 - c12 * c12;
    const double p3 = a13 * (a23 * s31 - a13 * s23);
    const double p2 = 2.0 * blob * a23 * a13 + a13 * (2.0 * a12 + a13) * s23 + a23 * (a23 - a12) * s31;
    const double p1 = a23 * (a13 - a23) * s12 - a12 * a12 * s23 - 2.0 * a12 * (blob * a23 + a13 * s23);
    const double p0 = a12 * (a12 * s23 - a23 * s12);
    if (!(fabs(p3) > 0)) return 0;
    const double g = pr_cubic_root(p2 / p3, p1 / p3, p0 / p3);
    double A[9];
    A[0] = a23 * (1.0 - g);
    A[1] = (a23 * b12) * 0.5;
    A[2] = (a23 * b13 * g) * (-0.5);
    A[4] = a23 - a12 + a13 * g;
    A[5] = b23 * (a13 * g - a12) * 0.5;
    A[8] = g * (a13 - a23) - a12;
    A[3] = A[1]; A[6] = A[2]; A[7] = A[5];
    double V[6], L[2];
    pr_eig_known0(A, V, L);
    const double q = -L[1] / L[0];
    const double v = q > 0 ? sqrt(q) : 0.0;
    double X[9], Xi[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) { X[k * 3 + 0] = d12[k]; X[k * 3 + 1] = d13[k]; X[k * 3 + 2] = nx[k]; }
    ygz_inv3(X, Xi);
    int cnt = 0;
#pragma unroll
    for (int si = 0; si < 2; ++si) {
        const double s = si == 0 ? v : -v;
        const double w2 = 1.0 / (s * V[3] - V[0]);
        const double w0 = (V[1] - s * V[4]) * w2;
        const double w1 = (V[2] - s * V[5]) * w2;
        const double a = 1.0 / ((a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12);
        const double b = (a13 * b12 * w1 - a12 * b13 * w0 - 2.0 * w0 * w1 * (a12 - a13)) * a;
        const double c = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * a;
        double tau[2];
        if (!root2real(b, c, &tau[0], &tau[1])) continue;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
            if (!(tau[ti] > 0)) continue;
            const double d = a23 / (tau[ti] * (b23 + tau[ti]) + 1.0);
            if (!(d > 0)) continue;
            double l[3];
            l[1] = sqrt(d);
            l[2] = tau[ti] * l[1];
            l[0] = w0 * l[1] + w1 * l[2];
            if (!(l[0] >= 0)) continue;
            pr_refine(l, a12, a13, a23, b12, b13, b23);
            double P[12];
            if (!pose_from_depths(l, y1, y2, y3, x1, Xi, P)) continue;
#pragma unroll
            for (int k = 0; k < 12; ++k) sol[cnt * 12 + k] = P[k];
            ++cnt;
        }
    }
    return cnt;
}

__device__ __forceinline__ int pr_is_inlier(const double *P, double w0, double w1, double w2, double u, double v, const double *K4, double chi2)
{
    const double X = P[0] * w0 + P[1] * w1 + P[2] * w2 + P[9];
    const double Y = P[3] * w0 + P[4] * w1 + P[5] * w2 + P[10];
    const double Z = P[6] * w0 + P[7] * w1 + P[8] * w2 + P[11];
    if (!(Z > 0)) return 0;
    const double du = K4[0] * (X / Z) + K4[2] - u;
    const double dv = K4[1] * (Y / Z) + K4[3] - v;
    return du * du + dv * dv <= chi2;
}

}  // namespace

// ---- kernels -------------------------------------------------------------------------------------------------------------------
namespace ygz_pnp {

// grid (samples / 64, problems)
__global__ __launch_bounds__(PNP_SOLVE_LANES) void k_pnp_solve(PnpDev D)
{
    const int p = blockIdx.y, it = D.in->max_iter;
    const int s = blockIdx.x * PNP_SOLVE_LANES + threadIdx.x;
    if (s >= it) return;
    const int off = D.off[p];
    const size_t h = (size_t)p * it + s;
    if (D.skip && D.skip[p]) {                                           // a problem its caller's kernel left out: no hypothesis
        double *none = D.sol + h * 48;
        for (int k = 0; k < 48; ++k) none[k] = 0.0;
        D.nsol[h] = 0;
        return;
    }
    double w[9], x[6];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = off + D.sets[h * 3 + j];
        w[3 * j] = D.pw[3 * i]; w[3 * j + 1] = D.pw[3 * i + 1]; w[3 * j + 2] = D.pw[3 * i + 2];
        x[2 * j] = D.px[2 * i]; x[2 * j + 1] = D.px[2 * i + 1];
    }
    double *sol = D.sol + h * 48;
    const int ns = pr_p3p(w, x, D.in->K4, sol);
    for (int k = ns * 12; k < 48; ++k) sol[k] = 0.0;
    D.nsol[h] = ns;
}

// grid (4 * max_iter / 256, problems): lane = hypothesis, the problem's points in LDS tiles of 256
__global__ __launch_bounds__(PNP_SCORE_LANES) void k_pnp_score(PnpDev D)
{
    __shared__ double sw[3][PNP_SCORE_LANES], su[2][PNP_SCORE_LANES];
    const int p = blockIdx.y, it = D.in->max_iter;
    const int hyp = blockIdx.x * PNP_SCORE_LANES + threadIdx.x;
    const int off = D.off[p], n = (D.end ? D.end[p] : D.off[p + 1]) - off;
    const double chi2 = D.in->chi2;
    double K4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) K4[k] = D.in->K4[k];
    const size_t h = (size_t)p * it * 4 + hyp;
    const bool live = hyp < 4 * it && (hyp & 3) < D.nsol[(size_t)p * it + (hyp >> 2)];
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = live ? D.sol[h * 12 + k] : 0.0;
    int c = 0;
    for (int base = 0; base < n; base += PNP_SCORE_LANES) {
        const int m = min(PNP_SCORE_LANES, n - base);
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const int i = off + base + threadIdx.x;
            sw[0][threadIdx.x] = D.pw[3 * i]; sw[1][threadIdx.x] = D.pw[3 * i + 1]; sw[2][threadIdx.x] = D.pw[3 * i + 2];
            su[0][threadIdx.x] = D.px[2 * i]; su[1][threadIdx.x] = D.px[2 * i + 1];
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < m; ++j) c += pr_is_inlier(P, sw[0][j], sw[1][j], sw[2][j], su[0][j], su[1][j], K4, chi2);
    }
    if (hyp < 4 * it) D.counts[h] = c;
}

// block = problem: the winner (the largest key count << 32 | ~hypothesis), its pose and mask
__global__ __launch_bounds__(PNP_SEL_THREADS) void k_pnp_select(PnpDev D)
{
    __shared__ unsigned long long sh_key;
    __shared__ int sh_nh, sh_cnt;
    const int p = blockIdx.x, it = D.in->max_iter;
    if (threadIdx.x == 0) { sh_key = 0; sh_nh = 0; sh_cnt = 0; }
    __syncthreads();
    unsigned long long key = 0;
    int nh = 0;
    for (int hyp = threadIdx.x; hyp < 4 * it; hyp += PNP_SEL_THREADS) {
        const size_t h = (size_t)p * it * 4 + hyp;
        const int c = D.counts[h];
        if (c > 0) {
            const unsigned long long k = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(0xffffffffu - (uint32_t)hyp);
            if (k > key) key = k;
        }
        nh += (hyp & 3) < D.nsol[(size_t)p * it + (hyp >> 2)];
    }
    atomicMax(&sh_key, key);
    atomicAdd(&sh_nh, nh);
    __syncthreads();
    const unsigned long long best = sh_key;
    const int off = D.off[p], n = (D.end ? D.end[p] : D.off[p + 1]) - off;
    ygz_pnp_result *r = D.res + p;
    if (best == 0) {
        for (int i = threadIdx.x; i < n; i += PNP_SEL_THREADS) D.mask[off + i] = 0;
        if (threadIdx.x == 0) {
            for (int k = 0; k < 9; ++k) r->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
            for (int k = 0; k < 3; ++k) r->t[k] = 0.0;
            for (int k = 0; k < 7; ++k) r->T_cw[k] = k == 3 ? 1.0 : 0.0;
            r->success = 0; r->n_inliers = 0; r->best_sample = -1; r->best_solution = -1; r->n_hypotheses = sh_nh;
        }
        return;
    }
    const int hyp = (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu));
    const double *Pg = D.sol + ((size_t)p * it * 4 + hyp) * 12;
    double P[12], K4[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = Pg[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) K4[k] = D.in->K4[k];
    const double chi2 = D.in->chi2;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += PNP_SEL_THREADS) {
        const int j = off + i;
        const int in = pr_is_inlier(P, D.pw[3 * j], D.pw[3 * j + 1], D.pw[3 * j + 2], D.px[2 * j], D.px[2 * j + 1], K4, chi2);
        D.mask[j] = (uint8_t)in;
        c += in;
    }
    atomicAdd(&sh_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        double q[4];
        ygz_quat_from_matrix(P, q);
        for (int k = 0; k < 9; ++k) r->R[k] = P[k];
        for (int k = 0; k < 3; ++k) r->t[k] = P[9 + k];
        for (int k = 0; k < 4; ++k) r->T_cw[k] = q[k];
        for (int k = 0; k < 3; ++k) r->T_cw[4 + k] = P[9 + k];
        r->n_inliers = sh_cnt;
        r->success = sh_cnt >= D.in->min_inliers;
        r->best_sample = hyp >> 2; r->best_solution = hyp & 3;
        r->n_hypotheses = sh_nh;
    }
}

}  // namespace ygz_pnp

// ---- host side ----------------------------------------------------------------------------------------------------------------------
namespace {

static_assert(sizeof(PnpIn) == 56 && sizeof(ygz_pnp_result) == 176, "tests/cpp/blob_layout_host.cpp restates the block with these sizes");
struct Layout {
    size_t in, off, pw, px, sets, in_end;                    // the upload
    size_t res, mask, res_end, nsol, counts, sol, total;     // the copy back: [res, res_end) or [res, total)
};
Layout layout(int P, size_t N, int it)
{
    Layout L;
    YgzBlobLayout B;
    const size_t H = (size_t)P * it;                         // hypothesis sets
    L.in = B.add(sizeof(PnpIn));
    L.off = B.add_n<int32_t>((size_t)P + 1);
    L.pw = B.add_n<double>(N * 3);
    L.px = B.add_n<double>(N * 2);
    L.sets = B.add_n<int32_t>(H * 3);
    L.in_end = B.end;
    L.res = B.add_n<ygz_pnp_result>((size_t)P);
    L.mask = B.add(N);
    L.res_end = B.end;
    L.nsol = B.add_n<int32_t>(H);
    L.counts = B.add_n<int32_t>(H * 4);
    L.sol = B.add_n<double>(H * 4 * 12);
    L.total = B.end;
    return L;
}

// validation (before anything touches the device), one upload, the three launches, one copy back of [res, res_end) (all = false) or of
// [res, total), one wait; `out` receives the page-locked image of the block
int run(ygz_hip_ctx *ctx, int P, const int32_t *offsets, const double *pw, const double *px, const double *K4, const ygz_pnp_params *params,
        bool all, uint8_t **out, Layout *Lout)
{
    if (!ctx || !offsets || !pw || !px || !K4 || P < 1) return YGZ_E_INVALID;
    if (P > YGZ_PNP_MAX_PROBLEMS) return YGZ_E_CAPACITY;
    ygz_pnp_params p;
    if (params) p = *params; else ygz_hip_default_pnp_params(&p);
    if (p.max_iter < 1 || p.max_iter > YGZ_PNP_MAX_ITER || !(p.chi2 > 0)) return YGZ_E_INVALID;
    if (offsets[0] != 0) return YGZ_E_INVALID;
    bool big = false;
    for (int q = 0; q < P; ++q) {
        const int n = offsets[q + 1] - offsets[q];
        if (n < 4) return YGZ_E_INVALID;
        big = big || n > ctx->cells;
    }
    if (big) return YGZ_E_CAPACITY;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    const int it = p.max_iter;
    const size_t N = (size_t)offsets[P];
    const Layout L = layout(P, N, it);
    const size_t down_end = all ? L.total : L.res_end;       // [0, in_end) goes up, [res, down_end) comes back
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_PNP, L.total, down_end, &b);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = b.host, *dev = b.dev;
    PnpIn in;
    memset(&in, 0, sizeof in);
    for (int k = 0; k < 4; ++k) in.K4[k] = K4[k];
    in.chi2 = p.chi2; in.n_problems = P; in.max_iter = it; in.min_inliers = p.min_inliers;
    memcpy(up + L.in, &in, sizeof in);
    memcpy(up + L.off, offsets, (size_t)(P + 1) * 4);
    memcpy(up + L.pw, pw, N * 24);
    memcpy(up + L.px, px, N * 16);
    for (int q = 0; q < P; ++q)
        memcpy(up + L.sets + (size_t)q * it * 12, ygz_cvrng_cached_sets(offsets[q + 1] - offsets[q], it, 3).data(), (size_t)it * 12);
    if ((rc = ygz_blob_upload(ctx, b, L.in_end)) != YGZ_OK) return rc;
    PnpDev D;
    D.in = ygz_at<const PnpIn>(dev, L.in); D.off = ygz_at<const int32_t>(dev, L.off); D.pw = ygz_at<const double>(dev, L.pw);
    D.px = ygz_at<const double>(dev, L.px); D.sets = ygz_at<const int32_t>(dev, L.sets);
    D.res = ygz_at<ygz_pnp_result>(dev, L.res); D.mask = dev + L.mask; D.nsol = ygz_at<int32_t>(dev, L.nsol);
    D.counts = ygz_at<int32_t>(dev, L.counts); D.sol = ygz_at<double>(dev, L.sol);
    D.end = nullptr; D.skip = nullptr;
    YGZ_LAUNCH(ctx, KID_COUNT, k_pnp_solve, dim3(ygz_div_up(it, PNP_SOLVE_LANES), P), dim3(PNP_SOLVE_LANES), D);
    YGZ_LAUNCH(ctx, KID_COUNT, k_pnp_score, dim3(ygz_div_up(4 * it, PNP_SCORE_LANES), P), dim3(PNP_SCORE_LANES), D);
    YGZ_LAUNCH(ctx, KID_COUNT, k_pnp_select, dim3(P), dim3(PNP_SEL_THREADS), D);
    if ((rc = ygz_blob_fetch(ctx, b, L.res, down_end)) != YGZ_OK) return rc;
    *out = up;
    *Lout = L;
    return YGZ_OK;
}

}  // namespace

extern "C" {

void ygz_hip_default_pnp_params(ygz_pnp_params *p)
{
    if (!p) return;
    p->max_iter = 300; p->chi2 = 5.991; p->min_inliers = 10;
}

int ygz_hip_pnp_sample_sets(int n, int max_iter, int32_t *sets)
{
    if (n < 4 || max_iter < 1 || max_iter > YGZ_PNP_MAX_ITER || !sets) return YGZ_E_INVALID;
    ygz_cvrng_sample_sets(n, max_iter, 3, sets);
    return YGZ_OK;
}

int ygz_hip_pnp_ransac(ygz_hip_ctx *ctx, int n_problems, const int32_t *offsets, const double *pw, const double *px, const double K4[4],
                       const ygz_pnp_params *params, ygz_pnp_result *results, uint8_t *inliers)
{
    if (!results) return YGZ_E_INVALID;
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, n_problems, offsets, pw, px, K4, params, false, &o, &L);
    if (rc != YGZ_OK) return rc;
    memcpy(results, o + L.res, (size_t)n_problems * sizeof(ygz_pnp_result));
    if (inliers) memcpy(inliers, o + L.mask, (size_t)offsets[n_problems]);
    return YGZ_OK;
}

int ygz_hip_pnp_hypotheses(ygz_hip_ctx *ctx, const double *pw, const double *px, int n, const double K4[4], const ygz_pnp_params *params,
                           double *solutions, int32_t *n_solutions, int32_t *counts)
{
    const int32_t off[2] = { 0, n };
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, 1, off, pw, px, K4, params, true, &o, &L);
    if (rc != YGZ_OK) return rc;
    const int it = params ? params->max_iter : 300;
    if (solutions) memcpy(solutions, o + L.sol, (size_t)it * 4 * 12 * 8);
    if (n_solutions) memcpy(n_solutions, o + L.nsol, (size_t)it * 4);
    if (counts) memcpy(counts, o + L.counts, (size_t)it * 16);
    return YGZ_OK;
}

}  // extern "C"
