// Loop detection's geometric check -- Sim3 RANSAC and 7-dof refinement over several independent 3D-3D problems (one per loop candidate
// keyframe).  Nothing in the reference: LocalMapping.cpp:330 ends in a comment ("put this keyframe into the loop-detection queue"), as
// ORB-SLAM2's LoopClosing::ComputeSim3 does it.  The arithmetic is tests/sim3_ref.c's decision by decision (-ffp-contract=off, only + - * /
// and sqrt), so every output is bit-identical to it.  One call = one upload, four launches on the context's stream,
// one copy back, one wait:
//   k_sim3_solve    lane = (problem, sample): Horn's closed form on the sample's 3 correspondences (4x4 Jacobi), S12 and S21
//   k_sim3_score    lane = (problem, sample), the problem's pairs staged in LDS: the inlier count
//   k_sim3_select   block = problem: the highest count (ties: smallest sample), the winner's mask (bit 0)
//   k_sim3_refine   block = problem: g2o's LM on the winner's inliers (Optimizer::OptimizeSim3's schedule), the refined mask (bit 1)
#include "ygz_internal.h"
#include "posemath_dev.h"
#include <cstring>

#define SIM3_SOLVE_LANES 64                // k_sim3_solve
#define SIM3_SCORE_LANES 256               // k_sim3_score: samples per block = pairs per LDS tile
#define SIM3_SEL_THREADS 256               // k_sim3_select
#define SIM3_REF_LANES 256                 // k_sim3_refine: the lanes of the fixed summation order (SR_LANES of tests/sim3_ref.c)
#define SR_SWEEPS 8
#define SR_DMAX 1.7976931348623157e308

namespace {

struct Sim3In {
    double K4[4];
    double chi2, chi2_refine;
    int32_t n_problems, max_iter, min_inliers, iters_first, iters_more, iters_again, fix_scale, pad;
};

struct Sim3Dev {
    const Sim3In *in;
    const int32_t *off;                       // [P + 1]
    const double *X1, *X2, *px1, *px2;        // [N][3], [N][3], [N][2], [N][2]
    const int32_t *lv;                        // [N][2]
    const int32_t *sets;                      // [P][max_iter][3]
    // the block that is copied back
    ygz_sim3_result *res;                     // [P]
    uint8_t *mask;                            // [N]
    int32_t *valid;                           // [P][max_iter]
    int32_t *counts;                          // [P][max_iter]
    double *hyp;                              // [P][max_iter][16]
};

// ---- the arithmetic (tests/sim3_ref.c, function by function; rotation, Sim3 inverse and retraction: posemath_dev.h) ----------------
__device__ __forceinline__ void sim3_act(const double *S, const double *R, const double *X, double *P)
{
    double r[3];
    ygz_mat3_vec(R, X, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) P[k] = S[7] * r[k] + S[4 + k];
}

template <int p, int q>
__device__ __forceinline__ void jacobi_rot(double *A, double *V)
{
    const double apq = A[p * 4 + q];
    if (apq == 0.0) return;
    const double theta = (A[q * 4 + q] - A[p * 4 + p]) / (2.0 * apq);
    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0) t = -t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[p * 4 + p] = A[p * 4 + p] - t * apq;
    A[q * 4 + q] = A[q * 4 + q] + t * apq;
    A[p * 4 + q] = 0.0; A[q * 4 + p] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r == p || r == q) continue;
        const double arp = A[r * 4 + p], arq = A[r * 4 + q];
        const double np = c * arp - s * arq, nq = s * arp + c * arq;
        A[r * 4 + p] = np; A[p * 4 + r] = np;
        A[r * 4 + q] = nq; A[q * 4 + r] = nq;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double vrp = V[r * 4 + p], vrq = V[r * 4 + q];
        V[r * 4 + p] = c * vrp - s * vrq;
        V[r * 4 + q] = s * vrp + c * vrq;
    }
}

__device__ __forceinline__ void sr_jacobi4(double *A, double *V)
{
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sw = 0; sw < SR_SWEEPS; ++sw) {
        jacobi_rot<0, 1>(A, V); jacobi_rot<0, 2>(A, V); jacobi_rot<0, 3>(A, V);
        jacobi_rot<1, 2>(A, V); jacobi_rot<1, 3>(A, V); jacobi_rot<2, 3>(A, V);
    }
}

// Horn on 3 correspondences (sr_horn with n = 3)
__device__ __forceinline__ int sr_horn3(const double *X1, const double *X2, int fix_scale, double *S12, double *S21)
{
    double O1[3] = { 0, 0, 0 }, O2[3] = { 0, 0, 0 };
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) { O1[k] += X1[3 * i + k]; O2[k] += X2[3 * i + k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { O1[k] = O1[k] / 3; O2[k] = O2[k] / 3; }
    double M[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double a[3], b[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[k] = X2[3 * i + k] - O2[k]; b[k] = X1[3 * i + k] - O1[k]; }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) M[3 * r + c] += a[r] * b[c];
    }
    double N[16];
    N[0] = M[0] + M[4] + M[8];
    N[1] = M[5] - M[7];
    N[2] = M[6] - M[2];
    N[3] = M[1] - M[3];
    N[5] = M[0] - M[4] - M[8];
    N[6] = M[1] + M[3];
    N[7] = M[6] + M[2];
    N[10] = -M[0] + M[4] - M[8];
    N[11] = M[5] + M[7];
    N[15] = -M[0] - M[4] + M[8];
    N[4] = N[1]; N[8] = N[2]; N[12] = N[3]; N[9] = N[6]; N[13] = N[7]; N[14] = N[11];
    double V[16];
    sr_jacobi4(N, V);
    // the largest eigenvalue (ties: the smallest index), its column of V, without a run-time index into a register array
    double w = V[0], x = V[4], y = V[8], z = V[12], ev = N[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (N[i * 5] > ev) { ev = N[i * 5]; w = V[i]; x = V[4 + i]; y = V[8 + i]; z = V[12 + i]; }
    const double nq = sqrt(w * w + x * x + y * y + z * z);
    w = w / nq; x = x / nq; y = y / nq; z = z / nq;
    if (w < 0) { w = -w; x = -x; y = -y; z = -z; }
    S12[0] = x; S12[1] = y; S12[2] = z; S12[3] = w;
    double R[9];
    ygz_quat_rotation(S12, R);
    double s = 1.0;
    if (!fix_scale) {
        double num = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double a[3], b[3], r[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { a[k] = X2[3 * i + k] - O2[k]; b[k] = X1[3 * i + k] - O1[k]; }
            ygz_mat3_vec(R, a, r);
            num += b[0] * r[0] + b[1] * r[1] + b[2] * r[2];
            den += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        }
        s = num / den;
    }
    S12[7] = s;
    double ro[3];
    ygz_mat3_vec(R, O2, ro);
#pragma unroll
    for (int k = 0; k < 3; ++k) S12[4 + k] = O1[k] - s * ro[k];
    ygz_sim3_inverse(S12, S21);
    int ok = s > 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) ok &= fabs(S12[k]) <= SR_DMAX && fabs(S21[k]) <= SR_DMAX;
    return ok;
}

__device__ __forceinline__ int sr_collinear(const double *X)
{
    double d12[3], d13[3], nx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d12[k] = X[k] - X[3 + k]; d13[k] = X[k] - X[6 + k]; }
    nx[0] = d12[1] * d13[2] - d12[2] * d13[1];
    nx[1] = d12[2] * d13[0] - d12[0] * d13[2];
    nx[2] = d12[0] * d13[1] - d12[1] * d13[0];
    const double a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double nn = nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2];
    return !(nn > 1e-10 * a12 * a13);
}

__device__ __forceinline__ double sr_sigma2(int level)
{
    double s2 = 1.0;
    for (int k = 0; k < level; ++k) s2 = s2 * 4.0;
    return s2;
}

__device__ __forceinline__ double reproj2(const double *P, double u0, double u1, const double *K4, int *front)
{
    *front = P[2] > 0;
    const double du = K4[0] * (P[0] / P[2]) + K4[2] - u0;
    const double dv = K4[1] * (P[1] / P[2]) + K4[3] - u1;
    return du * du + dv * dv;
}

__device__ __forceinline__ int sr_is_inlier(const double *S12, const double *R12, const double *S21, const double *R21, const double *X1,
                                            const double *X2, const double *u1, const double *u2, const double *K4, double th1, double th2)
{
    double P[3], Q[3];
    int f1, f2;
    sim3_act(S12, R12, X2, P);
    sim3_act(S21, R21, X1, Q);
    const double e1 = reproj2(P, u1[0], u1[1], K4, &f1);
    const double e2 = reproj2(Q, u2[0], u2[1], K4, &f2);
    return f1 && f2 && e1 < th1 && e2 < th2;
}

// ---- refinement terms ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void edge_jacobian(const double *P, const double *D, const double *K4, double *J)
{
    const double iz = 1.0 / P[2];
    const double a = K4[0] * iz, b = K4[1] * iz;
    const double c = -(K4[0] * P[0]) * (iz * iz), d = -(K4[1] * P[1]) * (iz * iz);
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        J[k] = -(a * D[k] + c * D[14 + k]);
        J[7 + k] = -(b * D[7 + k] + d * D[14 + k]);
    }
}

// S, R (its rotation), Si, Ri (the inverse's): computed once per LM evaluation by the caller
__device__ __forceinline__ void sr_pair_terms(const double *S, const double *R, const double *Si, const double *Ri, const double *X1, const double *X2,
                                             const double *u1, const double *u2, int l1, int l2, const double *K4, int fix_scale, double *e12,
                                             double *e21, double *J12, double *J21, double *c12, double *c21)
{
    double P[3], Q[3], D[21];
    sim3_act(S, R, X2, P);
    sim3_act(Si, Ri, X1, Q);
    e12[0] = u1[0] - (K4[0] * (P[0] / P[2]) + K4[2]);
    e12[1] = u1[1] - (K4[1] * (P[1] / P[2]) + K4[3]);
    e21[0] = u2[0] - (K4[0] * (Q[0] / Q[2]) + K4[2]);
    e21[1] = u2[1] - (K4[1] * (Q[1] / Q[2]) + K4[3]);
    const double G1[21] = { 0.0, P[2], -P[1], 1.0, 0.0, 0.0, P[0],
                            -P[2], 0.0, P[0], 0.0, 1.0, 0.0, P[1],
                            P[1], -P[0], 0.0, 0.0, 0.0, 1.0, P[2] };
#pragma unroll
    for (int k = 0; k < 21; ++k) D[k] = G1[k];
    if (fix_scale) D[6] = D[13] = D[20] = 0.0;
    edge_jacobian(P, D, K4, J12);
    const double G2[21] = { 0.0, -X1[2], X1[1], -1.0, 0.0, 0.0, -X1[0],
                            X1[2], 0.0, -X1[0], 0.0, -1.0, 0.0, -X1[1],
                            -X1[1], X1[0], 0.0, 0.0, 0.0, -1.0, -X1[2] };
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 7; ++k) D[7 * r + k] = Si[7] * (Ri[3 * r] * G2[k] + Ri[3 * r + 1] * G2[7 + k] + Ri[3 * r + 2] * G2[14 + k]);
    if (fix_scale) D[6] = D[13] = D[20] = 0.0;
    edge_jacobian(Q, D, K4, J21);
    const double i1 = 1.0 / sr_sigma2(l1), i2 = 1.0 / sr_sigma2(l2);
    *c12 = (e12[0] * e12[0] + e12[1] * e12[1]) * i1;
    *c21 = (e21[0] * e21[0] + e21[1] * e21[1]) * i2;
}

__device__ __forceinline__ double huber(double c, double delta, double d2, double *w)
{
    if (c <= d2) { *w = 1.0; return c; }
    const double sq = sqrt(c);
    *w = delta / sq;
    return 2.0 * delta * sq - d2;
}

__device__ __forceinline__ void add_edge(double *acc, const double *J, const double *e, double c, double info, double delta, double d2)
{
    double w;
    const double rho = huber(c, delta, d2, &w);
    const double wi = w * info;
    int m = 0;
#pragma unroll
    for (int a = 0; a < 7; ++a)
#pragma unroll
        for (int b = a; b < 7; ++b) acc[m++] += wi * (J[a] * J[b] + J[7 + a] * J[7 + b]);
#pragma unroll
    for (int a = 0; a < 7; ++a) acc[28 + a] -= wi * (J[a] * e[0] + J[7 + a] * e[1]);
    acc[35] += rho;
}

// (H + lambda I) x = b out of the 28 + 7 totals, factor and substitutions in one: with ygz_chol_factor and ygz_chol_solve_packed of
// posemath_dev.h the compiler orders the pivot tests differently and k_sim3_refine's code changes, so the loops stay written out here
__device__ __forceinline__ int sr_solve7(const double *tot, double lambda, int fix_scale, double *x)
{
    double A[49], L[49], y[7];
    ygz_sym_unpack<7>(tot, A);
#pragma unroll
    for (int a = 0; a < 7; ++a) A[a * 7 + a] = A[a * 7 + a] + lambda;
    double bb[7];
#pragma unroll
    for (int a = 0; a < 7; ++a) bb[a] = tot[28 + a];
    if (fix_scale) {
#pragma unroll
        for (int a = 0; a < 7; ++a) { A[a * 7 + 6] = 0.0; A[6 * 7 + a] = 0.0; }
        A[48] = 1.0; bb[6] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 49; ++k) L[k] = 0.0;
    int ok = 1;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        double d = A[j * 7 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j * 7 + k] * L[j * 7 + k];
        ok &= d > 0;
        const double ljj = sqrt(d);
        L[j * 7 + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 7; ++i) {
            double v = A[i * 7 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i * 7 + k] * L[j * 7 + k];
            L[i * 7 + j] = v / ljj;
        }
    }
    if (!ok) return 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        double v = bb[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i * 7 + k] * y[k];
        y[i] = v / L[i * 7 + i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; ++k) v -= L[k * 7 + i] * x[k];
        x[i] = v / L[i * 7 + i];
    }
    return 1;
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------
// grid (samples / 64, problems)
__global__ __launch_bounds__(SIM3_SOLVE_LANES) void k_sim3_solve(Sim3Dev D)
{
    const int p = blockIdx.y, it = D.in->max_iter;
    const int s = blockIdx.x * SIM3_SOLVE_LANES + threadIdx.x;
    if (s >= it) return;
    const int off = D.off[p];
    const size_t h = (size_t)p * it + s;
    double a[9], b[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int i = off + D.sets[h * 3 + j];
#pragma unroll
        for (int k = 0; k < 3; ++k) { a[3 * j + k] = D.X1[3 * i + k]; b[3 * j + k] = D.X2[3 * i + k]; }
    }
    double S12[8], S21[8];
    int ok = !sr_collinear(a) && !sr_collinear(b);
    if (ok) ok = sr_horn3(a, b, D.in->fix_scale, S12, S21);
    double *o = D.hyp + h * 16;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double id = (k == 3 || k == 7) ? 1.0 : 0.0;
        o[k] = ok ? S12[k] : id;
        o[8 + k] = ok ? S21[k] : id;
    }
    D.valid[h] = ok;
}

// grid (max_iter / 256, problems): lane = sample, the problem's pairs in LDS tiles of 256
__global__ __launch_bounds__(SIM3_SCORE_LANES) void k_sim3_score(Sim3Dev D)
{
    __shared__ double sx1[3][SIM3_SCORE_LANES], sx2[3][SIM3_SCORE_LANES], su1[2][SIM3_SCORE_LANES], su2[2][SIM3_SCORE_LANES];
    __shared__ double sth[2][SIM3_SCORE_LANES];
    const int p = blockIdx.y, it = D.in->max_iter;
    const int smp = blockIdx.x * SIM3_SCORE_LANES + threadIdx.x;
    const int off = D.off[p], n = D.off[p + 1] - off;
    const double chi2 = D.in->chi2;
    double K4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) K4[k] = D.in->K4[k];
    const size_t h = (size_t)p * it + smp;
    const bool live = smp < it && D.valid[h];
    double S12[8], S21[8], R12[9], R21[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) { S12[k] = live ? D.hyp[h * 16 + k] : 0.0; S21[k] = live ? D.hyp[h * 16 + 8 + k] : 0.0; }
    ygz_quat_rotation(S12, R12);
    ygz_quat_rotation(S21, R21);
    int c = 0;
    for (int base = 0; base < n; base += SIM3_SCORE_LANES) {
        const int m = min(SIM3_SCORE_LANES, n - base);
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const int i = off + base + threadIdx.x, t = threadIdx.x;
#pragma unroll
            for (int k = 0; k < 3; ++k) { sx1[k][t] = D.X1[3 * i + k]; sx2[k][t] = D.X2[3 * i + k]; }
#pragma unroll
            for (int k = 0; k < 2; ++k) { su1[k][t] = D.px1[2 * i + k]; su2[k][t] = D.px2[2 * i + k]; }
            sth[0][t] = chi2 * sr_sigma2(D.lv[2 * i]);
            sth[1][t] = chi2 * sr_sigma2(D.lv[2 * i + 1]);
        }
        __syncthreads();
        if (live)
            for (int j = 0; j < m; ++j) {
                const double x1[3] = { sx1[0][j], sx1[1][j], sx1[2][j] }, x2[3] = { sx2[0][j], sx2[1][j], sx2[2][j] };
                const double u1[2] = { su1[0][j], su1[1][j] }, u2[2] = { su2[0][j], su2[1][j] };
                c += sr_is_inlier(S12, R12, S21, R21, x1, x2, u1, u2, K4, sth[0][j], sth[1][j]);
            }
    }
    if (smp < it) D.counts[h] = c;
}

// block = problem: the winner (the largest key count << 32 | ~sample), its S12 / S21 and mask (bit 0); the refinement's fields zero
__global__ __launch_bounds__(SIM3_SEL_THREADS) void k_sim3_select(Sim3Dev D)
{
    __shared__ unsigned long long sh_key;
    __shared__ int sh_nh, sh_cnt;
    const int p = blockIdx.x, it = D.in->max_iter;
    if (threadIdx.x == 0) { sh_key = 0; sh_nh = 0; sh_cnt = 0; }
    __syncthreads();
    unsigned long long key = 0;
    int nh = 0;
    for (int s = threadIdx.x; s < it; s += SIM3_SEL_THREADS) {
        const size_t h = (size_t)p * it + s;
        const int c = D.counts[h];
        if (c > 0) {
            const unsigned long long k = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(0xffffffffu - (uint32_t)s);
            if (k > key) key = k;
        }
        nh += D.valid[h] != 0;
    }
    atomicMax(&sh_key, key);
    atomicAdd(&sh_nh, nh);
    __syncthreads();
    const unsigned long long best = sh_key;
    const int off = D.off[p], n = D.off[p + 1] - off;
    ygz_sim3_result *r = D.res + p;
    if (best == 0) {
        for (int i = threadIdx.x; i < n; i += SIM3_SEL_THREADS) D.mask[off + i] = 0;
        if (threadIdx.x == 0) {
            for (int k = 0; k < 8; ++k) { const double id = (k == 3 || k == 7) ? 1.0 : 0.0; r->S12[k] = id; r->S21[k] = id; }
            r->chi2_ransac = 0.0; r->chi2_refined = 0.0;
            r->success = 0; r->n_hypotheses = sh_nh; r->best_sample = -1; r->n_inliers = 0; r->n_refined = 0; r->lm_iterations = 0;
        }
        return;
    }
    const int smp = (int)(0xffffffffu - (uint32_t)(best & 0xffffffffu));
    const double *hg = D.hyp + ((size_t)p * it + smp) * 16;
    double S12[8], S21[8], R12[9], R21[9], K4[4];
#pragma unroll
    for (int k = 0; k < 8; ++k) { S12[k] = hg[k]; S21[k] = hg[8 + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) K4[k] = D.in->K4[k];
    ygz_quat_rotation(S12, R12);
    ygz_quat_rotation(S21, R21);
    const double chi2 = D.in->chi2;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += SIM3_SEL_THREADS) {
        const int j = off + i;
        const int in = sr_is_inlier(S12, R12, S21, R21, D.X1 + 3 * j, D.X2 + 3 * j, D.px1 + 2 * j, D.px2 + 2 * j, K4, chi2 * sr_sigma2(D.lv[2 * j]),
                                    chi2 * sr_sigma2(D.lv[2 * j + 1]));
        D.mask[j] = (uint8_t)in;
        c += in;
    }
    atomicAdd(&sh_cnt, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 8; ++k) { r->S12[k] = S12[k]; r->S21[k] = S21[k]; }
        r->chi2_ransac = 0.0; r->chi2_refined = 0.0;
        r->success = 0; r->n_hypotheses = sh_nh; r->best_sample = smp; r->n_inliers = sh_cnt; r->n_refined = 0; r->lm_iterations = 0;
    }
}

// the refinement's block-wide sums: every lane's partial sums over the pairs i = lane, lane + 256, ... (those with mask & bit), then the
// tree over the lanes (stride 128, 64, ..., 1) in LDS chunks of 12 values; tot written by lane 0, visible to all on return
struct RefShared {
    double red[12][SIM3_REF_LANES];
    double totH[36], totE;
    double S[8], Sb[8], x[7];
    int ok, drops, nin;
};

template <bool WITH_H>
__device__ void ref_accumulate(const Sim3Dev &D, RefShared &sh, int off, int n, int bit, const double *K4, int fix_scale, double delta, double d2)
{
    __syncthreads();                                                  // S as lane 0 last wrote it
    const int tid = threadIdx.x;
    double S[8], R[9], Si[8], Ri[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = sh.S[k];
    ygz_quat_rotation(S, R);
    ygz_sim3_inverse(S, Si);
    ygz_quat_rotation(Si, Ri);
    double acc[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += SIM3_REF_LANES) {
        const int j = off + i;
        if (!(D.mask[j] & bit)) continue;
        double e12[2], e21[2], J12[14], J21[14], c12, c21;
        const int l1 = D.lv[2 * j], l2 = D.lv[2 * j + 1];
        sr_pair_terms(S, R, Si, Ri, D.X1 + 3 * j, D.X2 + 3 * j, D.px1 + 2 * j, D.px2 + 2 * j, l1, l2, K4, fix_scale, e12, e21, J12, J21, &c12, &c21);
        if (WITH_H) {
            add_edge(acc, J12, e12, c12, 1.0 / sr_sigma2(l1), delta, d2);
            add_edge(acc, J21, e21, c21, 1.0 / sr_sigma2(l2), delta, d2);
        } else {
            double w;
            acc[35] += huber(c12, delta, d2, &w);
            acc[35] += huber(c21, delta, d2, &w);
        }
    }
    if (WITH_H) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 12; ++k) sh.red[k][tid] = acc[12 * ch + k];
            __syncthreads();
            for (int st = SIM3_REF_LANES / 2; st >= 1; st >>= 1) {
                if (tid < st)
#pragma unroll
                    for (int k = 0; k < 12; ++k) sh.red[k][tid] += sh.red[k][tid + st];
                __syncthreads();
            }
            if (tid == 0)
#pragma unroll
                for (int k = 0; k < 12; ++k) sh.totH[12 * ch + k] = sh.red[k][0];
        }
    } else {
        __syncthreads();
        sh.red[0][tid] = acc[35];
        __syncthreads();
        for (int st = SIM3_REF_LANES / 2; st >= 1; st >>= 1) {
            if (tid < st) sh.red[0][tid] += sh.red[0][tid + st];
            __syncthreads();
        }
        if (tid == 0) sh.totE = sh.red[0][0];
    }
    __syncthreads();
}

// one optimize(iters) of g2o's LM (sr_lm): every lane runs the same control flow on the block-wide sums; lane 0 solves and updates S
__device__ double ref_lm(const Sim3Dev &D, RefShared &sh, int off, int n, int bit, int iters, const double *K4, int fix_scale, double delta,
                         double d2, double *chi0, int *its)
{
    const int tid = threadIdx.x;
    double lambda = 0.0, ni = 2.0, currentChi = 0.0;
    for (int it = 0; it < iters; ++it) {
        ref_accumulate<true>(D, sh, off, n, bit, K4, fix_scale, delta, d2);
        currentChi = sh.totH[35];
        if (it == 0) {
            *chi0 = currentChi;
            double mx = 0.0;
            int m = 0;
            for (int a = 0; a < 7; ++a) { const double h = fabs(sh.totH[m]); if (h > mx) mx = h; m += 7 - a; }
            lambda = 1e-5 * mx; ni = 2.0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            __syncthreads();
            if (tid == 0) {
                double x[7], Sn[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) sh.Sb[k] = sh.S[k];
                int ok = sr_solve7(sh.totH, lambda, fix_scale, x);
                if (ok) ok = ygz_sim3_retract(sh.Sb, x, Sn);
                if (ok)
#pragma unroll
                    for (int k = 0; k < 8; ++k) sh.S[k] = Sn[k];
#pragma unroll
                for (int k = 0; k < 7; ++k) sh.x[k] = x[k];
                sh.ok = ok;
            }
            __syncthreads();
            const int ok = sh.ok;
            double tempChi = SR_DMAX;
            if (ok) {
                ref_accumulate<false>(D, sh, off, n, bit, K4, fix_scale, delta, d2);
                tempChi = sh.totE;
            }
            rho = currentChi - tempChi;
            double scale = 0.0;
            if (ok)
                for (int d = 0; d < 7; ++d) scale += sh.x[d] * (lambda * sh.x[d] + sh.totH[28 + d]);
            scale += 1e-3;
            rho = rho / scale;
            if (rho > 0 && fabs(tempChi) <= SR_DMAX) {
                const double u = 2.0 * rho - 1.0;
                double alpha = 1.0 - u * u * u;
                if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                lambda = lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
                ni = 2.0; currentChi = tempChi;
            } else {
                lambda = lambda * ni; ni = ni * 2.0;
                __syncthreads();
                if (tid == 0)
#pragma unroll
                    for (int k = 0; k < 8; ++k) sh.S[k] = sh.Sb[k];
                if (!(fabs(lambda) <= SR_DMAX)) break;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);
        ++*its;
        if (qmax == 10 || rho == 0 || !(fabs(lambda) <= SR_DMAX)) break;
    }
    return currentChi;
}

// every lane over its pairs with mask & 1 (first) or & 2 (second): the pairs with both chi2 <= chi2_refine at S get bit 1, the others lose it;
// the count of those dropped (first) or kept (second) into sh.drops / sh.nin
__device__ void ref_classify(const Sim3Dev &D, RefShared &sh, int off, int n, bool first, const double *K4, int fix_scale, double d2)
{
    __syncthreads();
    if (threadIdx.x == 0) { sh.drops = 0; sh.nin = 0; }
    __syncthreads();
    double S[8], R[9], Si[8], Ri[9];
#pragma unroll
    for (int k = 0; k < 8; ++k) S[k] = sh.S[k];
    ygz_quat_rotation(S, R);
    ygz_sim3_inverse(S, Si);
    ygz_quat_rotation(Si, Ri);
    int dr = 0, in = 0;
    for (int i = threadIdx.x; i < n; i += SIM3_REF_LANES) {
        const int j = off + i;
        const uint8_t m = D.mask[j];
        if (!(m & (first ? 1 : 2))) continue;
        double e12[2], e21[2], J12[14], J21[14], c12, c21;
        sr_pair_terms(S, R, Si, Ri, D.X1 + 3 * j, D.X2 + 3 * j, D.px1 + 2 * j, D.px2 + 2 * j, D.lv[2 * j], D.lv[2 * j + 1], K4, fix_scale, e12, e21,
                      J12, J21, &c12, &c21);
        const bool keep = c12 <= d2 && c21 <= d2;
        if (first) {
            if (keep) D.mask[j] = m | 2;
            else ++dr;
        } else {
            if (!keep) D.mask[j] = m & (uint8_t)~2u;
            else ++in;
        }
    }
    atomicAdd(&sh.drops, dr);
    atomicAdd(&sh.nin, in);
    __syncthreads();
}

// block = problem: Optimizer::OptimizeSim3's schedule on the RANSAC winner when it has min_inliers
__global__ __launch_bounds__(SIM3_REF_LANES) void k_sim3_refine(Sim3Dev D)
{
    __shared__ RefShared sh;
    const int p = blockIdx.x;
    ygz_sim3_result *r = D.res + p;
    const Sim3In &in = *D.in;
    if (r->best_sample < 0 || r->n_inliers < in.min_inliers) return;
    const int off = D.off[p], n = D.off[p + 1] - off;
    double K4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) K4[k] = in.K4[k];
    const double d2 = in.chi2_refine, delta = sqrt(d2);
    if (threadIdx.x == 0)
        for (int k = 0; k < 8; ++k) sh.S[k] = r->S12[k];
    int its = 0;
    double chi0 = 0.0, tmp = 0.0;
    ref_lm(D, sh, off, n, 1, in.iters_first, K4, in.fix_scale, delta, d2, &chi0, &its);
    ref_classify(D, sh, off, n, true, K4, in.fix_scale, d2);
    const double chi = ref_lm(D, sh, off, n, 2, sh.drops > 0 ? in.iters_more : in.iters_again, K4, in.fix_scale, delta, d2, &tmp, &its);
    ref_classify(D, sh, off, n, false, K4, in.fix_scale, d2);
    if (threadIdx.x == 0) {
        double S[8], Si[8];
        for (int k = 0; k < 8; ++k) S[k] = sh.S[k];
        ygz_sim3_inverse(S, Si);
        for (int k = 0; k < 8; ++k) { r->S12[k] = S[k]; r->S21[k] = Si[k]; }
        r->chi2_ransac = chi0;
        r->chi2_refined = chi;
        r->lm_iterations = its;
        r->n_refined = sh.nin;
        r->success = sh.nin >= in.min_inliers;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct Layout {
    size_t in, off, x1, x2, p1, p2, lv, sets, in_end;                 // the upload
    size_t res, mask, res_end, valid, counts, hyp, total;             // the copy back: [res, res_end) or [res, total)
};
Layout layout(int P, size_t N, int it)
{
    Layout L;
    YgzBlobLayout B;
    const size_t H = (size_t)P * it;                         // hypothesis sets
    L.in = B.add(sizeof(Sim3In));
    L.off = B.add_n<int32_t>((size_t)P + 1);
    L.x1 = B.add_n<double>(N * 3);
    L.x2 = B.add_n<double>(N * 3);
    L.p1 = B.add_n<double>(N * 2);
    L.p2 = B.add_n<double>(N * 2);
    L.lv = B.add_n<int32_t>(N * 2);
    L.sets = B.add_n<int32_t>(H * 3);
    L.in_end = B.end;
    L.res = B.add_n<ygz_sim3_result>((size_t)P);
    L.mask = B.add(N);
    L.res_end = B.end;
    L.valid = B.add_n<int32_t>(H);
    L.counts = B.add_n<int32_t>(H);
    L.hyp = B.add_n<double>(H * 16);
    L.total = B.end;
    return L;
}

// validation (before anything touches the device), one upload, the four launches, one copy back of [res, res_end) (all = false) or of
// [res, total), one wait; `out` receives the page-locked image of the block
int run(ygz_hip_ctx *ctx, int P, const int32_t *offsets, const double *X1, const double *X2, const double *px1, const double *px2,
        const int32_t *levels, const double *K4, const ygz_sim3_params *params, bool all, uint8_t **out, Layout *Lout)
{
    if (!ctx || !offsets || !X1 || !X2 || !px1 || !px2 || !levels || !K4 || P < 1) return YGZ_E_INVALID;
    if (P > YGZ_SIM3_MAX_PROBLEMS) return YGZ_E_CAPACITY;
    ygz_sim3_params p;
    if (params) p = *params; else ygz_hip_default_sim3_params(&p);
    if (p.max_iter < 1 || p.max_iter > YGZ_SIM3_MAX_ITER || !(p.chi2 > 0) || !(p.chi2_refine > 0) || p.iters_first < 0 || p.iters_more < 0
        || p.iters_again < 0)
        return YGZ_E_INVALID;
    if (offsets[0] != 0) return YGZ_E_INVALID;
    bool big = false;
    for (int q = 0; q < P; ++q) {
        const int n = offsets[q + 1] - offsets[q];
        if (n < 3) return YGZ_E_INVALID;
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
    int rc = ygz_blob_open(ctx, SCR_SIM3, L.total, down_end, &b);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = b.host, *dev = b.dev;
    Sim3In in;
    memset(&in, 0, sizeof in);
    for (int k = 0; k < 4; ++k) in.K4[k] = K4[k];
    in.chi2 = p.chi2; in.chi2_refine = p.chi2_refine; in.n_problems = P; in.max_iter = it; in.min_inliers = p.min_inliers;
    in.iters_first = p.iters_first; in.iters_more = p.iters_more; in.iters_again = p.iters_again; in.fix_scale = p.fix_scale != 0;
    memcpy(up + L.in, &in, sizeof in);
    memcpy(up + L.off, offsets, (size_t)(P + 1) * 4);
    memcpy(up + L.x1, X1, N * 24);
    memcpy(up + L.x2, X2, N * 24);
    memcpy(up + L.p1, px1, N * 16);
    memcpy(up + L.p2, px2, N * 16);
    memcpy(up + L.lv, levels, N * 8);
    for (int q = 0; q < P; ++q)
        memcpy(up + L.sets + (size_t)q * it * 12, ygz_cvrng_cached_sets(offsets[q + 1] - offsets[q], it, 3).data(), (size_t)it * 12);
    if ((rc = ygz_blob_upload(ctx, b, L.in_end)) != YGZ_OK) return rc;
    Sim3Dev D;
    D.in = ygz_at<const Sim3In>(dev, L.in); D.off = ygz_at<const int32_t>(dev, L.off);
    D.X1 = ygz_at<const double>(dev, L.x1); D.X2 = ygz_at<const double>(dev, L.x2);
    D.px1 = ygz_at<const double>(dev, L.p1); D.px2 = ygz_at<const double>(dev, L.p2);
    D.lv = ygz_at<const int32_t>(dev, L.lv); D.sets = ygz_at<const int32_t>(dev, L.sets);
    D.res = ygz_at<ygz_sim3_result>(dev, L.res); D.mask = dev + L.mask; D.valid = ygz_at<int32_t>(dev, L.valid);
    D.counts = ygz_at<int32_t>(dev, L.counts); D.hyp = ygz_at<double>(dev, L.hyp);
    YGZ_LAUNCH(ctx, KID_COUNT, k_sim3_solve, dim3(ygz_div_up(it, SIM3_SOLVE_LANES), P), dim3(SIM3_SOLVE_LANES), D);
    YGZ_LAUNCH(ctx, KID_COUNT, k_sim3_score, dim3(ygz_div_up(it, SIM3_SCORE_LANES), P), dim3(SIM3_SCORE_LANES), D);
    YGZ_LAUNCH(ctx, KID_COUNT, k_sim3_select, dim3(P), dim3(SIM3_SEL_THREADS), D);
    YGZ_LAUNCH(ctx, KID_COUNT, k_sim3_refine, dim3(P), dim3(SIM3_REF_LANES), D);
    if ((rc = ygz_blob_fetch(ctx, b, L.res, down_end)) != YGZ_OK) return rc;
    *out = up;
    *Lout = L;
    return YGZ_OK;
}

}  // namespace

extern "C" {

void ygz_hip_default_sim3_params(ygz_sim3_params *p)
{
    if (!p) return;
    p->max_iter = 300; p->chi2 = 9.210; p->min_inliers = 20; p->chi2_refine = 10.0;
    p->iters_first = 5; p->iters_more = 10; p->iters_again = 5; p->fix_scale = 0;
}

int ygz_hip_sim3_ransac(ygz_hip_ctx *ctx, int n_problems, const int32_t *offsets, const double *X1, const double *X2, const double *px1,
                        const double *px2, const int32_t *levels, const double K4[4], const ygz_sim3_params *params, ygz_sim3_result *results,
                        uint8_t *inliers)
{
    if (!results) return YGZ_E_INVALID;
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, n_problems, offsets, X1, X2, px1, px2, levels, K4, params, false, &o, &L);
    if (rc != YGZ_OK) return rc;
    memcpy(results, o + L.res, (size_t)n_problems * sizeof(ygz_sim3_result));
    if (inliers) memcpy(inliers, o + L.mask, (size_t)offsets[n_problems]);
    return YGZ_OK;
}

int ygz_hip_sim3_hypotheses(ygz_hip_ctx *ctx, const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels,
                            int n, const double K4[4], const ygz_sim3_params *params, double *hyps, int32_t *valid, int32_t *counts)
{
    const int32_t off[2] = { 0, n };
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, 1, off, X1, X2, px1, px2, levels, K4, params, true, &o, &L);
    if (rc != YGZ_OK) return rc;
    const int it = params ? params->max_iter : 300;
    if (hyps) memcpy(hyps, o + L.hyp, (size_t)it * 16 * 8);
    if (valid) memcpy(valid, o + L.valid, (size_t)it * 4);
    if (counts) memcpy(counts, o + L.counts, (size_t)it * 4);
    return YGZ_OK;
}

}  // extern "C"
