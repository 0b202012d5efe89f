// Monocular initialisation -- Initializer::TryInitialize and what it calls (src/Algorithm/Initializer.cpp:9-965): H / F RANSAC over the
// reference's 8-point sample sets, model choice, ReconstructH / ReconstructF with CheckRT.  The arithmetic is tests/init_ref.c's decision
// by decision (the same one-sided Jacobi SVD, the same sums in the same order, -ffp-contract=off), so every output is bit-identical to it
// (DESIGN.md section 9).  One call = one upload, nine launches on the context's stream, one copy back, one wait:
//   k_init_normalize   Normalize (:140-175) of both point sets: the two sums walk the points in index order on one lane each
//   k_init_models      lane = (hypothesis, model): the 16 x 9 / 8 x 9 DLT system in LDS, Jacobi, F's rank-2 projection, denormalisation
//   k_init_score       lane = hypothesis, a block per 16 points: per-point chi2 contributions (CheckHomography :251-314,
//                      CheckFundamental :772-845), written point-major so the sums below read them coalesced
//   k_init_sum         lane = (hypothesis, model): the float score in point order (the reference's `score +=`)
//   k_init_select      first strict maximum of each model, rh, the model choice (:66-78), the winners' inlier masks
//   k_init_decompose   one lane: the 8 (H, :335-449) or 4 (F, :856-877) candidate motions and the camera matrices of CheckRT
//   k_init_checkrt     lane = (solution, point): Triangulate (4 x 4 Jacobi) and CheckRT's tests (:535-605)
//   k_init_parallax    block = solution: count and the 51st smallest float cos-parallax by rank (:607-614)
//   k_init_accept      the H / F acceptance rule (:462-500, :879-937), SE3(R21, t21), the accepted points
#include "ygz_internal.h"
#include "posemath_dev.h"
#include <cstring>
#include <mutex>
#include <map>
#include <tuple>
#include <vector>

#define INIT_MODEL_LANES 32                 // k_init_models: lanes per block (the DLT system and V of a lane: 225 doubles of LDS)
#define INIT_SCORE_PTS   16                 // k_init_score: points per block
#define INIT_SEL_THREADS 1024               // k_init_parallax

namespace {

// ---- the arithmetic (tests/init_ref.c, function by function; 3 x 3 inverse and matrix -> quaternion: posemath_dev.h) -----------------
#define IR_JACOBI_TOL 1e-15
#define IR_JACOBI_SWEEPS 40
template <int ST>
__device__ __forceinline__ void ir_jacobi(double *A, int m, int n, double *V)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[(i * n + j) * ST] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < IR_JACOBI_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < m; ++i) {
                    const double ap = A[(i * n + p) * ST], aq = A[(i * n + q) * ST];
                    alpha = alpha + ap * ap; beta = beta + aq * aq; gamma = gamma + ap * aq;
                }
                if (!(fabs(gamma) > IR_JACOBI_TOL * sqrt(alpha) * sqrt(beta))) continue;
                rotated = 1;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                double t;
                if (fabs(zeta) > 1e150) t = 1.0 / (2.0 * zeta);
                else t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < m; ++i) {
                    const double ap = A[(i * n + p) * ST], aq = A[(i * n + q) * ST];
                    A[(i * n + p) * ST] = c * ap - s * aq;
                    A[(i * n + q) * ST] = s * ap + c * aq;
                }
                for (int i = 0; i < n; ++i) {
                    const double vp = V[(i * n + p) * ST], vq = V[(i * n + q) * ST];
                    V[(i * n + p) * ST] = c * vp - s * vq;
                    V[(i * n + q) * ST] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
}

// index of the column of smallest norm after ir_jacobi: the last one of the smallest norm (what a stable decreasing sort puts last)
template <int ST>
__device__ __forceinline__ int ir_min_column(const double *W, int m, int n)
{
    int c = 0;
    double best = 0;
    for (int j = 0; j < n; ++j) {
        double s = 0;
        for (int i = 0; i < m; ++i) { const double w = W[(i * n + j) * ST]; s = s + w * w; }
        const double sv = sqrt(s);
        if (j == 0 || sv <= best) { c = j; best = sv; }
    }
    return c;
}

__device__ __forceinline__ double pick3(const double *a, int o) { return o == 0 ? a[0] : (o == 1 ? a[1] : a[2]); }

__device__ __forceinline__ void ir_svd3(const double *A, double *U, double *s, double *V)
{
    double W[9], Vj[9], sv[3]; int ord[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) W[k] = A[k];
    ir_jacobi<1>(W, 3, 3, Vj);
#pragma unroll
    for (int j = 0; j < 3; ++j) { double q = 0; for (int i = 0; i < 3; ++i) { const double w = W[i * 3 + j]; q = q + w * w; } sv[j] = sqrt(q); }
    // the stable insertion sort of three, decreasing
    int o0 = 0, o1 = 1, o2 = 2;
    if (pick3(sv, o1) > pick3(sv, o0)) { const int t = o0; o0 = o1; o1 = t; }
    if (pick3(sv, o2) > pick3(sv, o1)) { const int t = o1; o1 = o2; o2 = t; if (pick3(sv, o1) > pick3(sv, o0)) { const int u = o0; o0 = o1; o1 = u; } }
    ord[0] = o0; ord[1] = o1; ord[2] = o2;
    double Wo[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // the selects keep the arrays in registers (a run-time index would put them in scratch memory)
        const int o = ord[k];
        s[k] = o == 0 ? sv[0] : (o == 1 ? sv[1] : sv[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            V[i * 3 + k] = o == 0 ? Vj[i * 3] : (o == 1 ? Vj[i * 3 + 1] : Vj[i * 3 + 2]);
            Wo[i * 3 + k] = o == 0 ? W[i * 3] : (o == 1 ? W[i * 3 + 1] : W[i * 3 + 2]);
        }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) U[i * 3 + k] = Wo[i * 3 + k] / s[k];
    U[0 * 3 + 2] = U[1 * 3 + 0] * U[2 * 3 + 1] - U[2 * 3 + 0] * U[1 * 3 + 1];
    U[1 * 3 + 2] = U[2 * 3 + 0] * U[0 * 3 + 1] - U[0 * 3 + 0] * U[2 * 3 + 1];
    U[2 * 3 + 2] = U[0 * 3 + 0] * U[1 * 3 + 1] - U[1 * 3 + 0] * U[0 * 3 + 1];
    const double d = U[0 * 3 + 2] * Wo[0 * 3 + 2] + U[1 * 3 + 2] * Wo[1 * 3 + 2] + U[2 * 3 + 2] * Wo[2 * 3 + 2];
    if (d < 0)
#pragma unroll
        for (int i = 0; i < 3; ++i) V[i * 3 + 2] = -V[i * 3 + 2];
}

__device__ __forceinline__ void mul3(const double *a, const double *b, double *r)
{
    double t[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = t[k];
}
__device__ __forceinline__ void mul3t(const double *a, const double *b, double *r)
{
    double t[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) t[i * 3 + j] = a[i * 3 + 0] * b[j * 3 + 0] + a[i * 3 + 1] * b[j * 3 + 1] + a[i * 3 + 2] * b[j * 3 + 2];
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = t[k];
}
__device__ __forceinline__ void tr3(const double *a, double *r)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r[i * 3 + j] = a[j * 3 + i];
}
__device__ __forceinline__ double ir_det3(const double *a)
{
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    return a[0] * c0 + a[1] * c1 + a[2] * c2;
}

__device__ __forceinline__ float ir_h_contrib(const double *H12, double u1, double v1, double u2, double v2, float invSigmaSquare, int *in)
{
    const float th = 5.991;
    const float w2in1inv = 1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]);
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { *in = 0; return 0.0f; }
    *in = 1;
    return th - chiSquare1;
}

__device__ __forceinline__ void ir_f_contrib(const float *f, double du1, double dv1, double du2, double dv2, float invSigmaSquare,
                                             float *c1, float *c2, int *in)
{
    const float th = 3.841, thScore = 5.991;
    const float u1 = du1, v1 = dv1, u2 = du2, v2 = dv2;
    int bIn = 1;
    const float a2 = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2_ = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2_;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = 0; *c1 = 0.0f; } else *c1 = thScore - chiSquare1;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1_ = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1_;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = 0; *c2 = 0.0f; } else *c2 = thScore - chiSquare2;
    *in = bIn;
}

__device__ __forceinline__ int ir_h_solutions(const double *H21, const double *K, double *Rs, double *ts)
{
    double invK[9], A[9], U[9], sg[3], V[9];
    ygz_inv3(K, invK);
    mul3(invK, H21, A); mul3(A, K, A);
    ir_svd3(A, U, sg, V);
    const double d1 = sg[0], d2 = sg[1], d3 = sg[2];
    const double s = ir_det3(U) * ir_det3(V);
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return 0;
    const float aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[] = { aux1, aux1, -aux1, -aux1 };
    const float x3[] = { aux3, -aux3, aux3, -aux3 };
    const float aux_stheta = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[] = { aux_stheta, -aux_stheta, -aux_stheta, aux_stheta };
    const float aux_sphi = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[] = { aux_sphi, -aux_sphi, -aux_sphi, aux_sphi };
    double sU[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) sU[k] = s * U[k];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double Rp[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, tp[3], R[9], t[3];
        if (i < 4) {
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp[0] = x1[i]; tp[1] = 0.0; tp[2] = -x3[i];
            for (int k = 0; k < 3; ++k) tp[k] = tp[k] * (d1 - d3);
        } else {
            const int j = i - 4;
            Rp[0] = cphi; Rp[2] = sphi[j]; Rp[4] = -1; Rp[6] = sphi[j]; Rp[8] = -cphi;
            tp[0] = x1[j]; tp[1] = 0; tp[2] = x3[j];
            for (int k = 0; k < 3; ++k) tp[k] = tp[k] * (d1 + d3);
        }
        mul3(sU, Rp, R); mul3t(R, V, R);
        for (int r = 0; r < 3; ++r) t[r] = U[r * 3 + 0] * tp[0] + U[r * 3 + 1] * tp[1] + U[r * 3 + 2] * tp[2];
        const double nr = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        for (int r = 0; r < 3; ++r) ts[3 * i + r] = t[r] / nr;
        for (int k = 0; k < 9; ++k) Rs[9 * i + k] = R[k];
    }
    return 1;
}

__device__ __forceinline__ void ir_decompose_e(const double *E, double *R1, double *R2, double *t)
{
    double U[9], s[3], V[9], UW[9];
    ir_svd3(E, U, s, V);
    for (int i = 0; i < 3; ++i) t[i] = U[i * 3 + 2];
    const double nr = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int i = 0; i < 3; ++i) t[i] = t[i] / nr;
    const double W[9] = { 0, -1, 0, 1, 0, 0, 0, 0, 1 }, Wt[9] = { 0, 1, 0, -1, 0, 0, 0, 0, 1 };
    mul3(U, W, UW); mul3t(UW, V, R1);
    if (ir_det3(R1) < 0) for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
    mul3(U, Wt, UW); mul3t(UW, V, R2);
    if (ir_det3(R2) < 0) for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
}

// ---- device layout of one call ----------------------------------------------------------------------------------------------------
struct InitIn {                       // uploaded (with px1, px2, sets and the given inlier mask behind it)
    double K4[4];
    double min_parallax, ratio_h;
    double M[9];                      // ygz_hip_init_reconstruct: the given model
    float  sigma, sigma2;
    int    n, max_iter, min_triangulated, model_in;   // model_in 0: the model chosen by k_init_select
};
struct InitRec {                      // reconstruction state (device only)
    double M[9];
    double R[8][9], t[8][3];
    double P1[12], P2[8][12], O2[8][3];
    double par[8];
    int    model, ns, N, cnt[8];
};
struct InitDev {
    const InitIn *in;
    const double *px1, *px2;
    const int32_t *sets;
    const uint8_t *inl_in;
    double *pn1, *pn2, *T;            // T: T1, T2inv, T2t [27]
    double *H12;                      // [it][9]
    float  *contrib;                  // [n][3 * it]: H, F image 2, F image 1
    InitRec *rec;
    double *p3d;                      // [8][n][3]
    float  *cosv;                     // [8][n]
    uint8_t *flags;                   // [8][n]: bit 0 counted, bit 1 good
    // the block that is copied back
    ygz_init_result *res;
    double *pts3d;                    // [n][3]
    uint8_t *tri;                     // [n]
    uint8_t *inl_h, *inl_f;           // [n]
    float *score_h, *score_f;         // [it]
    double *H21, *F21;                // [it][9]
};

__global__ __launch_bounds__(256) void k_init_normalize(InitDev D)
{
    __shared__ double sh[2][4];       // per image: mean x, mean y, sX, sY
    const int n = D.in->n;
    if (threadIdx.x == 0 || threadIdx.x == 64) {              // one lane per image walks the points in index order (:146-160)
        const double *px = threadIdx.x == 0 ? D.px1 : D.px2;
        double m0 = 0, m1 = 0;
        for (int i = 0; i < n; ++i) { m0 = m0 + px[2 * i]; m1 = m1 + px[2 * i + 1]; }
        m0 = m0 / (double)n; m1 = m1 / (double)n;
        double d0 = 0, d1 = 0;
        for (int i = 0; i < n; ++i) { d0 = d0 + fabs(px[2 * i] - m0); d1 = d1 + fabs(px[2 * i + 1] - m1); }
        d0 = d0 / (double)n; d1 = d1 / (double)n;
        const float sX = 1.0 / d0, sY = 1.0 / d1;
        double *o = sh[threadIdx.x == 0 ? 0 : 1];
        o[0] = m0; o[1] = m1; o[2] = sX; o[3] = sY;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        D.pn1[2 * i] = (D.px1[2 * i] - sh[0][0]) * sh[0][2]; D.pn1[2 * i + 1] = (D.px1[2 * i + 1] - sh[0][1]) * sh[0][3];
        D.pn2[2 * i] = (D.px2[2 * i] - sh[1][0]) * sh[1][2]; D.pn2[2 * i + 1] = (D.px2[2 * i + 1] - sh[1][1]) * sh[1][3];
    }
    if (threadIdx.x == 0) {
        double T1[9], T2[9];
        for (int k = 0; k < 2; ++k) {
            double *T = k == 0 ? T1 : T2;
            const double m0 = sh[k][0], m1 = sh[k][1], sX = sh[k][2], sY = sh[k][3];
            T[0] = sX; T[1] = 0; T[2] = -m0 * sX; T[3] = 0; T[4] = sY; T[5] = -m1 * sY; T[6] = 0; T[7] = 0; T[8] = 1;
        }
        double T2inv[9], T2t[9];
        ygz_inv3(T2, T2inv);
        tr3(T2, T2t);
        for (int k = 0; k < 9; ++k) { D.T[k] = T1[k]; D.T[9 + k] = T2inv[k]; D.T[18 + k] = T2t[k]; }
    }
}

__global__ __launch_bounds__(INIT_MODEL_LANES) void k_init_models(InitDev D)
{
    __shared__ double sA[16 * 9 * INIT_MODEL_LANES];
    __shared__ double sV[9 * 9 * INIT_MODEL_LANES];
    const int it = D.in->max_iter;
    const int g = blockIdx.x * INIT_MODEL_LANES + threadIdx.x;
    if (g >= 2 * it) return;
    const bool isH = g < it;
    const int h = isH ? g : g - it;
    double *A = sA + threadIdx.x, *V = sV + threadIdx.x;
    const int m = isH ? 16 : 8;
    for (int i = 0; i < 8; ++i) {
        const int idx = D.sets[h * 8 + i];
        const double u1 = D.pn1[2 * idx], v1 = D.pn1[2 * idx + 1], u2 = D.pn2[2 * idx], v2 = D.pn2[2 * idx + 1];
        if (isH) {                                           // ComputeH21 :200-227
            double *r0 = A + (2 * i) * 9 * INIT_MODEL_LANES, *r1 = A + (2 * i + 1) * 9 * INIT_MODEL_LANES;
            const int L = INIT_MODEL_LANES;
            r0[0 * L] = 0.0; r0[1 * L] = 0.0; r0[2 * L] = 0.0; r0[3 * L] = -u1; r0[4 * L] = -v1; r0[5 * L] = -1; r0[6 * L] = v2 * u1; r0[7 * L] = v2 * v1; r0[8 * L] = v2;
            r1[0 * L] = u1; r1[1 * L] = v1; r1[2 * L] = 1; r1[3 * L] = 0.0; r1[4 * L] = 0.0; r1[5 * L] = 0.0; r1[6 * L] = -u2 * u1; r1[7 * L] = -u2 * v1; r1[8 * L] = -u2;
        } else {                                             // ComputeF21 :735-751
            double *r = A + i * 9 * INIT_MODEL_LANES;
            const int L = INIT_MODEL_LANES;
            r[0 * L] = u2 * u1; r[1 * L] = u2 * v1; r[2 * L] = u2; r[3 * L] = v2 * u1; r[4 * L] = v2 * v1; r[5 * L] = v2; r[6 * L] = u1; r[7 * L] = v1; r[8 * L] = 1;
        }
    }
    ir_jacobi<INIT_MODEL_LANES>(A, m, 9, V);
    const int c = ir_min_column<INIT_MODEL_LANES>(A, m, 9);
    double x[9];
    for (int i = 0; i < 9; ++i) x[i] = V[(i * 9 + c) * INIT_MODEL_LANES];
    const double *T1 = D.T, *T2inv = D.T + 9, *T2t = D.T + 18;
    double T1r[9], Tl[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { T1r[k] = T1[k]; Tl[k] = isH ? T2inv[k] : T2t[k]; }
    double M[9];
    if (isH) {                                               // FindHomography :123-125
        mul3(Tl, x, M); mul3(M, T1r, M);
        double H12[9];
        ygz_inv3(M, H12);
#pragma unroll
        for (int k = 0; k < 9; ++k) { D.H21[h * 9 + k] = M[k]; D.H12[h * 9 + k] = H12[k]; }
    } else {                                                 // ComputeF21 :759-761, FindFundamental :702-703
        double U[9], s[3], Vf[9], UD[9], Fn[9];
        ir_svd3(x, U, s, Vf);
#pragma unroll
        for (int i = 0; i < 3; ++i) { UD[i * 3 + 0] = U[i * 3 + 0] * s[0]; UD[i * 3 + 1] = U[i * 3 + 1] * s[1]; UD[i * 3 + 2] = U[i * 3 + 2] * 0.0; }
        mul3t(UD, Vf, Fn);
        mul3(Tl, Fn, M); mul3(M, T1r, M);
#pragma unroll
        for (int k = 0; k < 9; ++k) D.F21[h * 9 + k] = M[k];
    }
}

__global__ __launch_bounds__(256) void k_init_score(InitDev D)
{
    const int it = D.in->max_iter, n = D.in->n;
    const int h = blockIdx.y * 256 + threadIdx.x;
    if (h >= it) return;
    const float invSigmaSquare = 1.0 / (D.in->sigma * D.in->sigma);
    double H12[9];
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { H12[k] = D.H12[h * 9 + k]; f[k] = D.F21[h * 9 + k]; }
    const int i0 = blockIdx.x * INIT_SCORE_PTS, i1 = min(n, i0 + INIT_SCORE_PTS);
    for (int i = i0; i < i1; ++i) {
        const double u1 = D.px1[2 * i], v1 = D.px1[2 * i + 1], u2 = D.px2[2 * i], v2 = D.px2[2 * i + 1];
        int in;
        float *row = D.contrib + (size_t)i * 3 * it;
        row[h] = ir_h_contrib(H12, u1, v1, u2, v2, invSigmaSquare, &in);
        float c1, c2;
        ir_f_contrib(f, u1, v1, u2, v2, invSigmaSquare, &c1, &c2, &in);
        row[it + h] = c1;
        row[2 * it + h] = c2;
    }
}

__global__ __launch_bounds__(64) void k_init_sum(InitDev D)
{
    const int it = D.in->max_iter, n = D.in->n;
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= 2 * it) return;
    const float *c = D.contrib;
    const size_t stride = (size_t)3 * it;
    float s = 0;
    if (g < it) {
        for (int i = 0; i < n; ++i) s += c[i * stride + g];
        D.score_h[g] = s;
    } else {
        const int h = g - it;
        for (int i = 0; i < n; ++i) { s += c[i * stride + it + h]; s += c[i * stride + 2 * it + h]; }
        D.score_f[h] = s;
    }
}

__global__ __launch_bounds__(256) void k_init_select(InitDev D)
{
    __shared__ int sh_best[2];
    const int it = D.in->max_iter, n = D.in->n;
    ygz_init_result *r = D.res;
    if (threadIdx.x == 0) {
        float bh = 0, bf = 0;
        int ih = -1, jf = -1;
        for (int k = 0; k < it; ++k) {
            const float sh = D.score_h[k], sf = D.score_f[k];
            if (sh > bh) { bh = sh; ih = k; }
            if (sf > bf) { bf = sf; jf = k; }
        }
        for (int k = 0; k < 9; ++k) { r->H21[k] = ih >= 0 ? D.H21[ih * 9 + k] : 0.0; r->F21[k] = jf >= 0 ? D.F21[jf * 9 + k] : 0.0; }
        r->score_h = bh; r->score_f = bf; r->best_h = ih; r->best_f = jf;
        r->rh = bh / (bh + bf);
        r->model = (bh + bf == 0) ? YGZ_INIT_NONE : (r->rh > 0.4 ? YGZ_INIT_H : YGZ_INIT_F);
        sh_best[0] = ih; sh_best[1] = jf;
    }
    __syncthreads();
    const int ih = sh_best[0], jf = sh_best[1];
    const float invSigmaSquare = 1.0 / (D.in->sigma * D.in->sigma);
    double H12[9];
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) { H12[k] = ih >= 0 ? D.H12[ih * 9 + k] : 0.0; f[k] = jf >= 0 ? (float)D.F21[jf * 9 + k] : 0.0f; }
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double u1 = D.px1[2 * i], v1 = D.px1[2 * i + 1], u2 = D.px2[2 * i], v2 = D.px2[2 * i + 1];
        int in = 0;
        if (ih >= 0) (void)ir_h_contrib(H12, u1, v1, u2, v2, invSigmaSquare, &in);
        D.inl_h[i] = (uint8_t)in;
        in = 0;
        float c1, c2;
        if (jf >= 0) ir_f_contrib(f, u1, v1, u2, v2, invSigmaSquare, &c1, &c2, &in);
        D.inl_f[i] = (uint8_t)in;
    }
}

__global__ __launch_bounds__(64) void k_init_decompose(InitDev D)
{
    __shared__ int sh_n;
    const int n = D.in->n;
    InitRec *R = D.rec;
    const int model_in = D.in->model_in;
    const int model = model_in ? model_in : D.res->model;
    const uint8_t *inl = model_in ? D.inl_in : (model == YGZ_INIT_H ? D.inl_h : D.inl_f);
    if (threadIdx.x == 0) sh_n = 0;
    __syncthreads();
    int c = 0;
    for (int i = threadIdx.x; i < n; i += 64) c += inl[i] != 0;
    atomicAdd(&sh_n, c);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double *K4 = D.in->K4;
    const double K[9] = { K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1 };
    double M[9];
    for (int k = 0; k < 9; ++k) M[k] = model_in ? D.in->M[k] : (model == YGZ_INIT_H ? D.res->H21[k] : D.res->F21[k]);
    R->model = model; R->N = sh_n;
    for (int k = 0; k < 9; ++k) R->M[k] = M[k];
    int ns = 0;
    if (model == YGZ_INIT_H) {
        ns = ir_h_solutions(M, K, &R->R[0][0], &R->t[0][0]) ? 8 : 0;
    } else if (model == YGZ_INIT_F) {                        // ReconstructF :856-877
        double Kt[9], E[9], R1[9], R2[9], t[3];
        tr3(K, Kt);
        mul3(Kt, M, E); mul3(E, K, E);
        ir_decompose_e(E, R1, R2, t);
        for (int k = 0; k < 9; ++k) { R->R[0][k] = R1[k]; R->R[1][k] = R2[k]; R->R[2][k] = R1[k]; R->R[3][k] = R2[k]; }
        for (int k = 0; k < 3; ++k) { R->t[0][k] = t[k]; R->t[1][k] = t[k]; R->t[2][k] = -t[k]; R->t[3][k] = -t[k]; }
        ns = 4;
    }
    R->ns = ns;
    for (int k = 0; k < 12; ++k) R->P1[k] = 0;                // CheckRT :522-532
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R->P1[i * 4 + j] = K[i * 3 + j];
    for (int s = 0; s < ns; ++s) {
        double Rt[12];
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) Rt[i * 4 + j] = R->R[s][i * 3 + j]; Rt[i * 4 + 3] = R->t[s][i]; }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) R->P2[s][i * 4 + j] = K[i * 3 + 0] * Rt[0 * 4 + j] + K[i * 3 + 1] * Rt[1 * 4 + j] + K[i * 3 + 2] * Rt[2 * 4 + j];
        for (int i = 0; i < 3; ++i) R->O2[s][i] = -R->R[s][0 * 3 + i] * R->t[s][0] + -R->R[s][1 * 3 + i] * R->t[s][1] + -R->R[s][2 * 3 + i] * R->t[s][2];
    }
}

__global__ __launch_bounds__(256) void k_init_checkrt(InitDev D)
{
    const InitRec *R = D.rec;
    const int s = blockIdx.y, n = D.in->n;
    if (s >= R->ns) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool isH = R->model == YGZ_INIT_H;
    const float th2 = isH ? (float)(4.0 * D.in->sigma2) : (float)(24.0 * D.in->sigma2);
    const double *K4 = D.in->K4;
    const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
    const double x1 = D.px1[2 * i], y1 = D.px1[2 * i + 1], x2 = D.px2[2 * i], y2 = D.px2[2 * i + 1];
    double A[16], V[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {                            // Triangulate :655-661
        A[0 * 4 + c] = x1 * R->P1[2 * 4 + c] - R->P1[0 * 4 + c];
        A[1 * 4 + c] = y1 * R->P1[2 * 4 + c] - R->P1[1 * 4 + c];
        A[2 * 4 + c] = x2 * R->P2[s][2 * 4 + c] - R->P2[s][0 * 4 + c];
        A[3 * 4 + c] = y2 * R->P2[s][2 * 4 + c] - R->P2[s][1 * 4 + c];
    }
    ir_jacobi<1>(A, 4, 4, V);
    const int col = ir_min_column<1>(A, 4, 4);
    double x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = col == 0 ? V[k * 4] : (col == 1 ? V[k * 4 + 1] : (col == 2 ? V[k * 4 + 2] : V[k * 4 + 3]));
    const double p0 = x[0] / x[3], p1 = x[1] / x[3], p2 = x[2] / x[3];
    uint8_t flag = 0;
    float cosf_ = 0;
    double o0 = 0, o1 = 0, o2 = 0;
    do {                                                     // CheckRT :539-604
        if (!isfinite(p0)) break;
        const double n2x = p0 - R->O2[s][0], n2y = p1 - R->O2[s][1], n2z = p2 - R->O2[s][2];
        const double dist1 = sqrt(p0 * p0 + p1 * p1 + p2 * p2);
        const double dist2 = sqrt(n2x * n2x + n2y * n2y + n2z * n2z);
        const double cosParallax = (p0 * n2x + p1 * n2y + p2 * n2z) / (dist1 * dist2);
        if (p2 < 0 && cosParallax < 0.99998) break;
        const double *Rm = R->R[s], *t = R->t[s];
        const double q0 = Rm[0] * p0 + Rm[1] * p1 + Rm[2] * p2 + t[0];
        const double q1 = Rm[3] * p0 + Rm[4] * p1 + Rm[5] * p2 + t[1];
        const double q2 = Rm[6] * p0 + Rm[7] * p1 + Rm[8] * p2 + t[2];
        if (q2 < 0 && cosParallax < 0.99998) break;
        if (isH) {
            const double invZ1 = 1.0 / p2;
            const double im1x = fx * p0 * invZ1 + cx, im1y = fy * p1 * invZ1 + cy;
            const double e1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
            if (e1 > th2) break;
            const double invZ2 = 1.0 / q2;
            const double im2x = fx * q0 * invZ2 + cx, im2y = fy * q1 * invZ2 + cy;
            const double e2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
            if (e2 > th2) break;
        }
        cosf_ = (float)cosParallax;
        o0 = p0; o1 = p1; o2 = p2;
        flag = 1 | (cosParallax < 0.99998 ? 2 : 0);
    } while (0);
    const size_t k = (size_t)s * n + i;
    D.p3d[3 * k] = o0; D.p3d[3 * k + 1] = o1; D.p3d[3 * k + 2] = o2;
    D.cosv[k] = cosf_;
    D.flags[k] = flag;
}

// count and the min(50, count - 1)-th smallest counted cos-parallax of one solution: the element whose rank (smaller values, plus equal
// values at lower indices) is that index -- the value the sort leaves there; NaN when a counted value is NaN (tests/init_ref.c ir_parallax)
__global__ __launch_bounds__(INIT_SEL_THREADS) void k_init_parallax(InitDev D)
{
    __shared__ int sh_cnt, sh_nan;
    InitRec *R = D.rec;
    const int s = blockIdx.x, n = D.in->n;
    if (s >= R->ns) return;
    const float *cv = D.cosv + (size_t)s * n;
    const uint8_t *fl = D.flags + (size_t)s * n;
    if (threadIdx.x == 0) { sh_cnt = 0; sh_nan = 0; }
    __syncthreads();
    int c = 0, nan_ = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (fl[i] & 1) { ++c; nan_ |= isnan(cv[i]) ? 1 : 0; }
    atomicAdd(&sh_cnt, c);
    if (nan_) atomicOr(&sh_nan, 1);
    __syncthreads();
    const int cnt = sh_cnt;
    if (threadIdx.x == 0) {
        R->cnt[s] = cnt;
        if (cnt <= 0) R->par[s] = 0;
        else if (sh_nan) R->par[s] = __builtin_nan("");
    }
    if (cnt <= 0 || sh_nan) return;
    const int idx = cnt - 1 < 50 ? cnt - 1 : 50;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (!(fl[i] & 1)) continue;
        const float v = cv[i];
        int rank = 0;
        for (int j = 0; j < n && rank <= idx; ++j)
            rank += ((fl[j] & 1) && (cv[j] < v || (cv[j] == v && j < i))) ? 1 : 0;
        if (rank == idx) {
            const float a = (float)acos((double)v);
            R->par[s] = (double)(a * 180.0f) / M_PI;
        }
    }
}

__global__ __launch_bounds__(256) void k_init_accept(InitDev D)
{
    __shared__ int sh_best, sh_ok, sh_tri;
    const InitRec *R = D.rec;
    const int n = D.in->n;
    ygz_init_result *r = D.res;
    if (threadIdx.x == 0) {
        const int ns = R->ns, model = R->model;
        const float minParallax = (float)D.in->min_parallax;
        const int min_triangulated = D.in->min_triangulated, N = R->N;
        int best = -1, accept = 0;
        r->n_inliers = N; r->success = 0; r->n_good = 0; r->second_good = 0; r->similar = 0; r->parallax = 0; r->n_triangulated = 0;
        if (model == YGZ_INIT_H && ns == 8) {                // ReconstructH :451-498
            int bestGood = 0, secondBestGood = 0;
            float bestParallax = -1;
            for (int i = 0; i < 8; ++i) {
                const int g = R->cnt[i];
                if (g > bestGood) { secondBestGood = bestGood; bestGood = g; best = i; bestParallax = R->par[i]; }
                else if (g > secondBestGood) secondBestGood = g;
            }
            r->n_good = bestGood; r->second_good = secondBestGood;
            r->parallax = best >= 0 ? R->par[best] : 0;
            accept = secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > min_triangulated
                     && bestGood > D.in->ratio_h * n;
        } else if (model == YGZ_INIT_F) {                    // ReconstructF :879-937
            int maxGood = R->cnt[0];
            for (int i = 1; i < 4; ++i) if (R->cnt[i] > maxGood) maxGood = R->cnt[i];
            const int ng = (int)(0.9 * N), minGood = ng > min_triangulated ? ng : min_triangulated;
            int similar = 0, second = 0;
            for (int i = 0; i < 4; ++i) if (R->cnt[i] > 0.7 * maxGood) ++similar;
            for (int i = 0; i < 4; ++i) if (best < 0 && R->cnt[i] == maxGood) best = i;
            for (int i = 0; i < 4; ++i) if (i != best && R->cnt[i] > second) second = R->cnt[i];
            r->n_good = maxGood; r->second_good = second; r->similar = similar; r->parallax = R->par[best];
            accept = !(maxGood < minGood || similar > 1) && R->par[best] > minParallax;
        }
        r->solution = best; r->model = model;
        for (int k = 0; k < 9; ++k) r->R21[k] = (k % 4 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 3; ++k) r->t21[k] = 0;
        if (accept) {
            r->success = 1;
            for (int k = 0; k < 9; ++k) r->R21[k] = R->R[best][k];
            for (int k = 0; k < 3; ++k) r->t21[k] = R->t[best][k];
        }
        double q[4], Rm[9];
        for (int k = 0; k < 9; ++k) Rm[k] = r->R21[k];
        ygz_quat_from_matrix(Rm, q);                          // _T21 = SE3(R21, t21) (:79)
        for (int k = 0; k < 4; ++k) r->T21[k] = q[k];
        for (int k = 0; k < 3; ++k) r->T21[4 + k] = r->t21[k];
        sh_best = best; sh_ok = accept; sh_tri = 0;
    }
    __syncthreads();
    const int best = sh_best, ok = sh_ok;
    int c = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const size_t k = ok ? (size_t)best * n + i : 0;
        const uint8_t f = ok ? D.flags[k] : 0;
        D.pts3d[3 * i] = ok ? D.p3d[3 * k] : 0.0; D.pts3d[3 * i + 1] = ok ? D.p3d[3 * k + 1] : 0.0; D.pts3d[3 * i + 2] = ok ? D.p3d[3 * k + 2] : 0.0;
        D.tri[i] = (f >> 1) & 1;
        c += (f >> 1) & 1;
    }
    atomicAdd(&sh_tri, c);
    __syncthreads();
    if (threadIdx.x == 0) r->n_triangulated = sh_tri;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
}  // namespace

// cv::RNG (OpenCV core/operations.hpp): default state 0xffffffff, next() multiply-with-carry, uniform(int a, int b) = next() % (b - a) + a.
// TryInitialize :33-48 draws k = 8 indices per iteration; the relocalisation's P3P (pnp.hip) draws k = 3 by the same scheme.
void ygz_cvrng_sample_sets(int n, int max_iter, int k, int32_t *sets)
{
    uint64_t st = 0xffffffffu;
    std::vector<int32_t> avail(n);
    for (int it = 0; it < max_iter; ++it) {
        int na = n;
        for (int i = 0; i < n; ++i) avail[i] = i;
        for (int j = 0; j < k; ++j) {
            st = (uint64_t)(uint32_t)st * 4164903690u + (uint32_t)(st >> 32);
            const int r = (int)((uint32_t)st % (uint32_t)na);
            sets[it * k + j] = avail[r];
            avail[r] = avail[na - 1];
            --na;
        }
    }
}

// the sets depend on (n, max_iter, k) only: drawn once per triple and kept
const std::vector<int32_t> &ygz_cvrng_cached_sets(int n, int max_iter, int k)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, std::vector<int32_t>> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto &v = cache[std::make_tuple(n, max_iter, k)];
    if (v.empty()) { v.resize((size_t)max_iter * k); ygz_cvrng_sample_sets(n, max_iter, k, v.data()); }
    return v;
}

namespace {

struct Layout {
    size_t in, px1, px2, sets, inl_in, in_end;             // the upload
    size_t res, pts3d, tri, inl_h, inl_f, score_h, score_f, H21, F21, out_end;   // the copy back
    size_t pn1, pn2, T, H12, contrib, rec, p3d, cosv, flags, total;
};
Layout layout(int n, int it)
{
    Layout L;
    YgzBlobLayout B;
    const size_t N = (size_t)n, I = (size_t)it;
    L.in = B.add(sizeof(InitIn));
    L.px1 = B.add_n<double>(N * 2);
    L.px2 = B.add_n<double>(N * 2);
    L.sets = B.add_n<int32_t>(I * 8);
    L.inl_in = B.add(N);
    L.in_end = B.end;
    L.res = B.add(sizeof(ygz_init_result));
    L.pts3d = B.add_n<double>(N * 3);
    L.tri = B.add(N);
    L.inl_h = B.add(N);
    L.inl_f = B.add(N);
    L.score_h = B.add_n<float>(I);
    L.score_f = B.add_n<float>(I);
    L.H21 = B.add_n<double>(I * 9);
    L.F21 = B.add_n<double>(I * 9);
    L.out_end = B.end;
    L.pn1 = B.add_n<double>(N * 2);
    L.pn2 = B.add_n<double>(N * 2);
    L.T = B.add_n<double>(27);
    L.H12 = B.add_n<double>(I * 9);
    L.contrib = B.add_n<float>(N * I * 3);
    L.rec = B.add(sizeof(InitRec));
    L.p3d = B.add_n<double>(8 * N * 3);
    L.cosv = B.add_n<float>(8 * N);
    L.flags = B.add(8 * N);
    L.total = B.end;
    return L;
}

InitDev bind(uint8_t *b, const Layout &L)
{
    InitDev D;
    D.in = ygz_at<const InitIn>(b, L.in); D.px1 = ygz_at<const double>(b, L.px1); D.px2 = ygz_at<const double>(b, L.px2);
    D.sets = ygz_at<const int32_t>(b, L.sets); D.inl_in = b + L.inl_in;
    D.pn1 = ygz_at<double>(b, L.pn1); D.pn2 = ygz_at<double>(b, L.pn2); D.T = ygz_at<double>(b, L.T); D.H12 = ygz_at<double>(b, L.H12);
    D.contrib = ygz_at<float>(b, L.contrib); D.rec = ygz_at<InitRec>(b, L.rec); D.p3d = ygz_at<double>(b, L.p3d);
    D.cosv = ygz_at<float>(b, L.cosv); D.flags = b + L.flags;
    D.res = ygz_at<ygz_init_result>(b, L.res); D.pts3d = ygz_at<double>(b, L.pts3d); D.tri = b + L.tri; D.inl_h = b + L.inl_h;
    D.inl_f = b + L.inl_f; D.score_h = ygz_at<float>(b, L.score_h); D.score_f = ygz_at<float>(b, L.score_f);
    D.H21 = ygz_at<double>(b, L.H21); D.F21 = ygz_at<double>(b, L.F21);
    return D;
}

enum { RUN_HYP = 1, RUN_REC = 2 };

// validation, one upload, the launches of `what`, one copy back of [res, out_end) (or of [res, inl_h) when only the reconstruction's
// outputs are wanted), one wait; `out` receives the page-locked image of the block
int run(ygz_hip_ctx *ctx, const double *px1, const double *px2, int n, const double *K4, const ygz_init_params *params, int what,
        int model_in, const double *M, const uint8_t *inl_in, uint8_t **out, Layout *Lout)
{
    YgzDeviceGuard dg_(ctx);
    if (!ctx || !px1 || !px2 || n < 8) return YGZ_E_INVALID;
    ygz_init_params p;
    if (params) p = *params; else ygz_hip_default_init_params(&p);
    if (p.max_iter < 1 || p.max_iter > YGZ_INIT_MAX_ITER || !(p.sigma > 0)) return YGZ_E_INVALID;
    if ((what & RUN_REC) && !K4) return YGZ_E_INVALID;
    if (model_in && (!M || !inl_in || (model_in != YGZ_INIT_H && model_in != YGZ_INIT_F))) return YGZ_E_INVALID;
    if (n > ctx->cells) return YGZ_E_CAPACITY;
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    const int it = p.max_iter;
    const Layout L = layout(n, it);
    YgzBlob b;                                               // [0, in_end) goes up, [res, out_end) comes back
    int rc = ygz_blob_open(ctx, SCR_INIT, L.total, L.out_end, &b);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = b.host, *dev = b.dev;
    InitIn in;
    memset(&in, 0, sizeof in);
    for (int k = 0; k < 4; ++k) in.K4[k] = K4 ? K4[k] : 0.0;
    in.min_parallax = p.min_parallax; in.ratio_h = p.good_point_ratio_h;
    for (int k = 0; k < 9; ++k) in.M[k] = M ? M[k] : 0.0;
    in.sigma = p.sigma; in.sigma2 = p.sigma2; in.n = n; in.max_iter = it; in.min_triangulated = p.min_triangulated; in.model_in = model_in;
    memcpy(up + L.in, &in, sizeof in);
    memcpy(up + L.px1, px1, (size_t)n * 16);
    memcpy(up + L.px2, px2, (size_t)n * 16);
    if (what & RUN_HYP) memcpy(up + L.sets, ygz_cvrng_cached_sets(n, it, 8).data(), (size_t)it * 32);
    if (inl_in) memcpy(up + L.inl_in, inl_in, (size_t)n);
    const size_t up_bytes = inl_in ? L.in_end : L.inl_in;
    if ((rc = ygz_blob_upload(ctx, b, up_bytes)) != YGZ_OK) return rc;
    YGZ_HIPCHK(ctx, hipMemsetAsync(dev + L.res, 0, sizeof(ygz_init_result), ctx->stream));
    const InitDev D = bind(dev, L);
    if (what & RUN_HYP) {
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_normalize, dim3(1), dim3(256), D);
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_models, dim3(ygz_div_up(2 * it, INIT_MODEL_LANES)), dim3(INIT_MODEL_LANES), D);
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_score, dim3(ygz_div_up(n, INIT_SCORE_PTS), ygz_div_up(it, 256)), dim3(256), D);
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_sum, dim3(ygz_div_up(2 * it, 64)), dim3(64), D);
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_select, dim3(1), dim3(256), D);
    }
    if (what & RUN_REC) {
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_decompose, dim3(1), dim3(64), D);
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_checkrt, dim3(ygz_div_up(n, 256), 8), dim3(256), D);
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_parallax, dim3(8), dim3(INIT_SEL_THREADS), D);
        YGZ_LAUNCH(ctx, KID_COUNT, k_init_accept, dim3(1), dim3(256), D);
    }
    const size_t down_end = (what & RUN_HYP) && !(what & RUN_REC) ? L.out_end : L.inl_h;
    if ((rc = ygz_blob_fetch(ctx, b, L.res, down_end)) != YGZ_OK) return rc;
    *out = up;
    *Lout = L;
    return YGZ_OK;
}

}  // namespace

extern "C" {

void ygz_hip_default_init_params(ygz_init_params *p)
{
    if (!p) return;
    p->sigma = 2.0f; p->sigma2 = 4.0f; p->max_iter = 200; p->min_parallax = 1.0; p->min_triangulated = 8; p->good_point_ratio_h = 0.9;
}

int ygz_hip_init_sample_sets(int n, int max_iter, int32_t *sets)
{
    if (n < 8 || max_iter < 1 || max_iter > YGZ_INIT_MAX_ITER || !sets) return YGZ_E_INVALID;
    ygz_cvrng_sample_sets(n, max_iter, 8, sets);
    return YGZ_OK;
}

int ygz_hip_initialize(ygz_hip_ctx *ctx, const double *px1, const double *px2, int n, const double K4[4], const ygz_init_params *params,
                       ygz_init_result *result, double *pts3d_out, uint8_t *triangulated_out)
{
    if (!result || !K4) return YGZ_E_INVALID;
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, px1, px2, n, K4, params, RUN_HYP | RUN_REC, 0, nullptr, nullptr, &o, &L);
    if (rc != YGZ_OK) return rc;
    memcpy(result, o + L.res, sizeof *result);
    if (pts3d_out) memcpy(pts3d_out, o + L.pts3d, (size_t)n * 24);
    if (triangulated_out) memcpy(triangulated_out, o + L.tri, (size_t)n);
    return YGZ_OK;
}

int ygz_hip_init_hypotheses(ygz_hip_ctx *ctx, const double *px1, const double *px2, int n, const ygz_init_params *params, double *H21,
                            double *F21, float *score_h, float *score_f, uint8_t *inliers_h, uint8_t *inliers_f, ygz_init_result *result)
{
    if (!result) return YGZ_E_INVALID;
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, px1, px2, n, nullptr, params, RUN_HYP, 0, nullptr, nullptr, &o, &L);
    if (rc != YGZ_OK) return rc;
    const int it = params ? params->max_iter : 200;
    memcpy(result, o + L.res, sizeof *result);
    if (H21) memcpy(H21, o + L.H21, (size_t)it * 72);
    if (F21) memcpy(F21, o + L.F21, (size_t)it * 72);
    if (score_h) memcpy(score_h, o + L.score_h, (size_t)it * 4);
    if (score_f) memcpy(score_f, o + L.score_f, (size_t)it * 4);
    if (inliers_h) memcpy(inliers_h, o + L.inl_h, (size_t)n);
    if (inliers_f) memcpy(inliers_f, o + L.inl_f, (size_t)n);
    return YGZ_OK;
}

int ygz_hip_init_reconstruct(ygz_hip_ctx *ctx, const double *px1, const double *px2, int n, const double K4[4], const ygz_init_params *params,
                             int model, const double M[9], const uint8_t *inliers, ygz_init_result *result, double *pts3d_out,
                             uint8_t *triangulated_out)
{
    if (!result || !K4 || (model != YGZ_INIT_H && model != YGZ_INIT_F)) return YGZ_E_INVALID;
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, px1, px2, n, K4, params, RUN_REC, model, M, inliers, &o, &L);
    if (rc != YGZ_OK) return rc;
    memcpy(result, o + L.res, sizeof *result);
    if (pts3d_out) memcpy(pts3d_out, o + L.pts3d, (size_t)n * 24);
    if (triangulated_out) memcpy(triangulated_out, o + L.tri, (size_t)n);
    return YGZ_OK;
}

}  // extern "C"
