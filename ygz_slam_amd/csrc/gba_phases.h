// The phases of the Schur-complement PCG Levenberg-Marquardt solver that do not see the edge model, and the host driver around them: shared by
// gba.hip (two residual rows per edge, ygz_hip_global_ba) and sba.hip (mono and stereo edges of up to three rows, ygz_hip_stereo_ba).  A file
// that includes this header defines GBA_LANES, GBA_CHUNK and GBA_CG_CAP first, wraps every gba_ph_* body in a kernel of its own and hands
// the driver its fifteen kernels (GbaKernels).  Only four phases read residuals and Jacobians -- the linearisation, the two system
// gathers and the trial cost; they live in the including file.  The other eleven work on Hpp, Hll, bp, bl and the 6 x 3 Hpl blocks alone.
#pragma once
#include "ygz_internal.h"
#include "posemath_dev.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

static_assert(GBA_LANES == 256 && GBA_CHUNK == 1024 && GBA_CG_CAP == 1024, "the summation order of tests/gba_ref.c and tests/sba_ref.c");
#define GBA_DEFAULT_BATCH 8                // CG iterations queued per read-back when cg_batch is 0
#define GB_DMAX 1.7976931348623157e308

namespace {

// the control state of the LM and CG loops; zero-filled at the upload, written only by the one-workgroup kernels (and by the integer
// atomics of the flags and of the diagonal maximum), read back by the host once per batch
struct GbaRec {
    double lambda, ni, currentChi, tempChi, cost_initial, rz, stop, rho;
    unsigned long long maxdiag_bits;          // the bits of the largest diagonal element (non-negative doubles order as integers)
    int32_t bad_lin, bad_trial, bad_cost;     // integer flags, atomicOr
    int32_t trial_ok, cg_done, cg_it, decided, accepted, finished, converged;
    int32_t status, qmax, lm_iterations, n_solves, cg_total, cg_capped, pad;
};

struct GbaIn {
    double K[4], delta, cg_tol, min_rel_decrease;
    int32_t n, nl, ne, max_iterations, max_trials, cg_cap, stage_only, pad;
    // sba.hip only: bf = fx * baseline, chi2_mono and chi2_stereo with their square roots; whether the Huber kernel is on in this round and
    // whether the outlier flags of the last classification switch edges off (every round but the first)
    double bf, d2m, d2s, dm, ds;
    int32_t robust, use_outliers;
};

struct GbaDev {
    const GbaIn *in;
    GbaRec *rec;
    const uint8_t *fixed;                     // [N]
    const int32_t *edge_pose, *edge_point;    // [E]
    const double *obs;                        // [E][2] (gba.hip), [E][3] (sba.hip)
    const uint8_t *kind;                      // sba.hip: [E] 0 absent, 1 mono, 2 stereo
    const int32_t *level;                     // sba.hip: [E]
    uint8_t *outlier;                         // sba.hip: [E] the flags of the last classification
    double *chi2;                             // sba.hip: [E]
    int32_t *ipart;                           // sba.hip: the inlier counts of the edge chunks
    const int32_t *pt_off, *pt_adj, *pt_pose; // [L + 1], [E] edges per point in edge-index order, [E] the pose of that slot (-1: fixed)
    const int32_t *ps_off, *ps_adj, *ps_point;// [N + 1], [E] edges per pose in edge-index order, [E] the point of that slot
    const int32_t *slot_l, *slot_p;           // [E] the edge's position in pt_adj and in ps_adj
    double *T, *X, *Tn, *Xn;                  // [N][7], [L][3]: the estimate and the trial
    double *res, *w, *Jp, *Jl;                // edge order, structure of arrays: [rows][E], [E], [6 rows][E], [3 rows][E]
    double *HplP, *HplL;                      // [18][E] in pose-slot order and in point-slot order
    double *cpart, *lpart;                    // chunk sums of the edges' cost terms and of the points' denominator terms
    double *Hpp, *bp, *bt, *Lf, *x, *r, *z, *p, *q, *vterm, *sterm;   // [N][21], [N][6], [N][6], [N][21], 5 x [N][6], [N], [N]
    double *Hll, *bl, *Hinv, *wl, *vl;        // structure of arrays over the points: [6][L], [3][L], [6][L], [3][L], [3][L]
};

template <int K> struct GbaRed {
    double red[K][GBA_LANES];
    double out[K];
};

// ---- the arithmetic (tests/gba_ref.c, function by function; its rotation, retraction and Cholesky loops are posemath_dev.h's) -----------
__device__ __forceinline__ int gb_residual(const double *T, const double *X, const double *ob, const double *K, double *R, double *P, double *r)
{
    ygz_quat_rotation(T, R);
#pragma unroll
    for (int i = 0; i < 3; ++i) P[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2]) + T[4 + i];
    if (!(P[2] > 0)) return 0;
    const double xn = P[0] / P[2], yn = P[1] / P[2];
    r[0] = ob[0] - (K[0] * xn + K[2]);
    r[1] = ob[1] - (K[1] * yn + K[3]);
    return fabs(r[0]) <= GB_DMAX && fabs(r[1]) <= GB_DMAX;
}

__device__ __forceinline__ void gb_robust(const double *r, double delta, double *rho0, double *rho1)
{
    const double e2 = r[0] * r[0] + r[1] * r[1], dsqr = delta * delta;
    *rho0 = e2; *rho1 = 1.0;
    if (delta > 0 && e2 > dsqr) {
        const double s = sqrt(e2);
        *rho0 = 2.0 * s * delta - dsqr;
        *rho1 = delta / s;
    }
}

__device__ __forceinline__ int gb_edge_terms(const double *T, const double *X, const double *ob, const double *K, double delta, double *r,
                                             double *w, double *rho, double *Jp, double *Jl)
{
    double R[9], P[3];
    if (!gb_residual(T, X, ob, K, R, P, r)) {
        r[0] = 0.0; r[1] = 0.0; *w = 0.0; *rho = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k) Jp[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) Jl[k] = 0.0;
        return 0;
    }
    gb_robust(r, delta, rho, w);
    const double x = P[0], y = P[1], z = P[2];
    const double iz = 1.0 / z, a = K[0] * iz, b = K[1] * iz, c = K[0] * (x / z) * iz, d = K[1] * (y / z) * iz;
    Jp[0] = c * y;         Jp[1] = -(a * z) - c * x; Jp[2] = a * y;    Jp[3] = -a;  Jp[4] = 0.0; Jp[5] = c;
    Jp[6] = b * z + d * y; Jp[7] = -(d * x);         Jp[8] = -(b * x); Jp[9] = 0.0; Jp[10] = -b; Jp[11] = d;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        Jl[k] = -(a * R[k]) + c * R[6 + k];
        Jl[3 + k] = -(b * R[3 + k]) + d * R[6 + k];
    }
    return 1;
}

__device__ __forceinline__ int gb_inv3(const double *A, double lambda, double *inv)
{
    const double a00 = A[0] + lambda, a01 = A[1], a02 = A[2], a11 = A[3] + lambda, a12 = A[4], a22 = A[5] + lambda;
    const double d0 = a00, l10 = a01 / d0, l20 = a02 / d0;
    const double d1 = a11 - l10 * a01, t21 = a12 - l20 * a01, l21 = t21 / d1;
    const double d2 = (a22 - l20 * a02) - l21 * t21;
    const double m20 = l10 * l21 - l20, i0 = 1.0 / d0, i1 = 1.0 / d1, i2 = 1.0 / d2;
    inv[0] = i0 + (l10 * l10) * i1 + (m20 * m20) * i2;
    inv[1] = -(l10 * i1) - (m20 * l21) * i2;
    inv[2] = m20 * i2;
    inv[3] = i1 + (l21 * l21) * i2;
    inv[4] = -(l21 * i2);
    inv[5] = i2;
    return d0 > 0 && d1 > 0 && d2 > 0;
}

__device__ __forceinline__ void gb_sym3_mul(const double *M, const double *v, double *o)
{
    o[0] = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
    o[1] = M[1] * v[0] + M[3] * v[1] + M[4] * v[2];
    o[2] = M[2] * v[0] + M[4] * v[1] + M[5] * v[2];
}

// gb_chol6 of tests/gba_ref.c: the packed upper triangle D, the packed lower factor Lo
__device__ __forceinline__ int gb_chol6(const double *D, double *Lo)
{
    double A[36];
    ygz_sym_unpack<6>(D, A);
    return ygz_chol_factor<6>(A, Lo);
}

// ---- sums ------------------------------------------------------------------------------------------------------------------------------
// gb_tree over the lanes' partial sums of K quantities at once: strides 128 and 64 out of LDS, 32 .. 1 inside a wavefront (lane l adds lane
// l + stride's, the same pairs as the tree); wavefront w takes the quantities w, w + 4, ...; two barriers; the totals are in sh.out
static_assert(GBA_LANES == 256, "gba_reduce spells the tree for 256 lanes");
template <int K> __device__ __forceinline__ void gba_reduce(GbaRed<K> &sh, const double *acc)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) sh.red[k][tid] = acc[k];
    __syncthreads();
    for (int k = wave; k < K; k += GBA_LANES / 64) {
        double v = (sh.red[k][lane] + sh.red[k][lane + 128]) + (sh.red[k][lane + 64] + sh.red[k][lane + 192]);
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) v += __shfl_down(v, st);
        if (lane == 0) sh.out[k] = v;
    }
    __syncthreads();
}

// gb_sum1 of v [n] by one workgroup: lane-strided in index order, then the tree; every lane returns the total
__device__ __forceinline__ double gba_sum1(GbaRed<1> &sh, const double *v, int n)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += GBA_LANES) acc += v[i];
    gba_reduce<1>(sh, &acc);
    return sh.out[0];
}

__device__ __forceinline__ bool gba_after_accept(const GbaRec *rec) { return rec->decided && rec->accepted && !rec->finished; }
__device__ __forceinline__ bool gba_in_tail(const GbaRec *rec) { return rec->cg_done && !rec->decided; }

// the largest diagonal element so far: positive doubles order as their bits do
__device__ __forceinline__ void gba_max_diag(GbaRec *rec, double h)
{
    h = fabs(h);
    if (h > 0) atomicMax(&rec->maxdiag_bits, (unsigned long long)__double_as_longlong(h));
}

__device__ __forceinline__ void gba_ph_begin(const GbaDev &D)
{
    __shared__ GbaRed<1> sh;
    const GbaIn &in = *D.in;
    GbaRec *rec = D.rec;
    const int bad = rec->bad_lin;
    const double cost = gba_sum1(sh, D.cpart, (in.ne + GBA_CHUNK - 1) / GBA_CHUNK);
    if (threadIdx.x != 0) return;
    const int ok = !bad && fabs(cost) <= GB_DMAX;
    rec->cost_initial = cost; rec->currentChi = cost;
    rec->lambda = ok ? 1e-5 * __longlong_as_double((long long)rec->maxdiag_bits) : 0.0;
    rec->ni = 2.0;
    rec->status = ok ? YGZ_GBA_MAX_ITERATIONS : YGZ_GBA_FAILED;
    rec->finished = !ok;
    rec->decided = 0; rec->accepted = 0; rec->cg_done = 1; rec->qmax = 0;
}

// ---- one trial of lambda ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gba_ph_point_trial(const GbaDev &D)
{
    const GbaIn &in = *D.in;
    const size_t L = (size_t)in.nl;
    const int l = blockIdx.x * GBA_LANES + threadIdx.x;
    if (l >= in.nl) return;
    double A[6], b[3], inv[6], wl[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) A[k] = D.Hll[k * L + l];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = D.bl[k * L + l];
    const int ok = gb_inv3(A, D.rec->lambda, inv);
    gb_sym3_mul(inv, b, wl);
#pragma unroll
    for (int k = 0; k < 6; ++k) D.Hinv[k * L + l] = inv[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) D.wl[k * L + l] = wl[k];
    if (!ok) atomicOr(&D.rec->bad_trial, 1);
}

__device__ __forceinline__ void gba_ph_pose_trial(const GbaDev &D)
{
    __shared__ GbaRed<27> sh;
    const int v = blockIdx.x;
    if (D.fixed[v]) return;
    const GbaIn &in = *D.in;
    const size_t E = (size_t)in.ne, L = (size_t)in.nl;
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int s = D.ps_off[v] + threadIdx.x; s < D.ps_off[v + 1]; s += GBA_LANES) {
        const size_t l = (size_t)D.ps_point[s];
        double H[18], Hi[6], wl[3], Tm[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) H[k] = D.HplP[k * E + s];
#pragma unroll
        for (int k = 0; k < 6; ++k) Hi[k] = D.Hinv[k * L + l];
#pragma unroll
        for (int k = 0; k < 3; ++k) wl[k] = D.wl[k * L + l];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            gb_sym3_mul(Hi, H + 3 * a, Tm + 3 * a);
            acc[21 + a] += H[3 * a] * wl[0] + H[3 * a + 1] * wl[1] + H[3 * a + 2] * wl[2];
        }
        int m = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[m++] += Tm[3 * a] * H[3 * b] + Tm[3 * a + 1] * H[3 * b + 1] + Tm[3 * a + 2] * H[3 * b + 2];
    }
    gba_reduce<27>(sh, acc);
    const int tid = threadIdx.x;
    if (tid >= 21 && tid < 27) D.bt[6 * v + tid - 21] = D.bp[6 * v + tid - 21] - sh.out[tid];
    if (tid == 0) {
        const double lambda = D.rec->lambda;
        double Dg[21], Lo[21];
        int m = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) {
                const double h = a == b ? D.Hpp[21 * v + m] + lambda : D.Hpp[21 * v + m];
                Dg[m] = h - sh.out[m];
                ++m;
            }
        const int ok = gb_chol6(Dg, Lo);
#pragma unroll
        for (int k = 0; k < 21; ++k) D.Lf[21 * v + k] = Lo[k];
        if (!ok) atomicOr(&D.rec->bad_trial, 1);
    }
}

// x = 0, r = bt, z = M^-1 r, p = z, r.z and the stop value; a non-positive pivot of the trial's blocks rejects the trial here, before CG
__device__ __forceinline__ void gba_ph_cg_begin(const GbaDev &D)
{
    __shared__ GbaRed<1> sh;
    const GbaIn &in = *D.in;
    GbaRec *rec = D.rec;
    const int bad = rec->bad_trial;
    double acc = 0.0;
    if (!bad)
        for (int v = threadIdx.x; v < in.n; v += GBA_LANES) {
            if (D.fixed[v]) continue;
            double r[6], z[6], Lo[21], d = 0.0;
#pragma unroll
            for (int k = 0; k < 21; ++k) Lo[k] = D.Lf[21 * v + k];
#pragma unroll
            for (int k = 0; k < 6; ++k) { r[k] = D.bt[6 * v + k]; D.x[6 * v + k] = 0.0; D.r[6 * v + k] = r[k]; }
            ygz_chol_solve_packed<6>(Lo, r, z);
#pragma unroll
            for (int k = 0; k < 6; ++k) { D.z[6 * v + k] = z[k]; D.p[6 * v + k] = z[k]; d += r[k] * z[k]; }
            acc += d;
        }
    gba_reduce<1>(sh, &acc);
    if (threadIdx.x != 0) return;
    rec->bad_trial = 0; rec->decided = 0; rec->accepted = 0; rec->cg_it = 0;
    if (bad) { rec->trial_ok = 0; rec->cg_done = 1; return; }
    const double rz = sh.out[0], stop = (in.cg_tol * in.cg_tol) * rz;
    rec->trial_ok = 1; rec->rz = rz; rec->stop = stop;
    ++rec->n_solves;
    rec->cg_done = rz <= stop;                                         // the cap is at least one iteration
}

// per point: sum over its edges with a free pose of Hpl^T y_pose, in edge-index order (gb_point_gather)
__device__ __forceinline__ void gba_point_gather(const GbaDev &D, const double *y, int l, size_t E, double *u)
{
    u[0] = 0.0; u[1] = 0.0; u[2] = 0.0;
    for (int s = D.pt_off[l]; s < D.pt_off[l + 1]; ++s) {
        const int j = D.pt_pose[s];
        if (j < 0) continue;
        double yj[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) yj[a] = y[6 * j + a];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double t = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) t += D.HplL[(3 * a + c) * E + s] * yj[a];
            u[c] += t;
        }
    }
}

__device__ __forceinline__ void gba_ph_cg_point(const GbaDev &D)
{
    if (D.rec->cg_done) return;
    const GbaIn &in = *D.in;
    const size_t L = (size_t)in.nl;
    const int l = blockIdx.x * GBA_LANES + threadIdx.x;
    if (l >= in.nl) return;
    double u[3], Hi[6], vl[3];
    gba_point_gather(D, D.p, l, (size_t)in.ne, u);
#pragma unroll
    for (int k = 0; k < 6; ++k) Hi[k] = D.Hinv[k * L + l];
    gb_sym3_mul(Hi, u, vl);
#pragma unroll
    for (int k = 0; k < 3; ++k) D.vl[k * L + l] = vl[k];
}

__device__ __forceinline__ void gba_ph_cg_pose(const GbaDev &D)
{
    __shared__ GbaRed<6> sh;
    if (D.rec->cg_done) return;
    const int v = blockIdx.x;
    if (D.fixed[v]) return;
    const GbaIn &in = *D.in;
    const size_t E = (size_t)in.ne, L = (size_t)in.nl;
    double acc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = 0.0;
    for (int s = D.ps_off[v] + threadIdx.x; s < D.ps_off[v + 1]; s += GBA_LANES) {
        const size_t l = (size_t)D.ps_point[s];
        const double v0 = D.vl[l], v1 = D.vl[L + l], v2 = D.vl[2 * L + l];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] += D.HplP[(3 * a) * E + s] * v0 + D.HplP[(3 * a + 1) * E + s] * v1 + D.HplP[(3 * a + 2) * E + s] * v2;
    }
    gba_reduce<6>(sh, acc);
    if (threadIdx.x != 0) return;
    const double lambda = D.rec->lambda;
    double A[36], p[6], d = 0.0;
    int m = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) { A[a * 6 + b] = D.Hpp[21 * v + m]; A[b * 6 + a] = D.Hpp[21 * v + m]; ++m; }
#pragma unroll
    for (int a = 0; a < 6; ++a) p[a] = D.p[6 * v + a];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < 6; ++b) t += A[a * 6 + b] * p[b];
        const double qa = (t + lambda * p[a]) - sh.out[a];
        D.q[6 * v + a] = qa;
        d += p[a] * qa;
    }
    D.vterm[v] = d;
}

__device__ __forceinline__ void gba_ph_cg_step(const GbaDev &D)
{
    __shared__ GbaRed<1> sh;
    GbaRec *rec = D.rec;
    if (rec->cg_done) return;
    const GbaIn &in = *D.in;
    const double rz = rec->rz, stop = rec->stop;
    const int it = rec->cg_it;
    const double pq = gba_sum1(sh, D.vterm, in.n);
    if (!(pq > 0)) {                                                   // CG ends with the iterate it has
        if (threadIdx.x == 0) { rec->cg_done = 1; rec->cg_total += it; }
        return;
    }
    const double alpha = rz / pq;
    double acc = 0.0;
    for (int v = threadIdx.x; v < in.n; v += GBA_LANES) {
        if (D.fixed[v]) continue;
        double r[6], z[6], Lo[21], d = 0.0;
#pragma unroll
        for (int k = 0; k < 21; ++k) Lo[k] = D.Lf[21 * v + k];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            D.x[6 * v + k] = D.x[6 * v + k] + alpha * D.p[6 * v + k];
            r[k] = D.r[6 * v + k] - alpha * D.q[6 * v + k];
            D.r[6 * v + k] = r[k];
        }
        ygz_chol_solve_packed<6>(Lo, r, z);
#pragma unroll
        for (int k = 0; k < 6; ++k) { D.z[6 * v + k] = z[k]; d += r[k] * z[k]; }
        acc += d;
    }
    gba_reduce<1>(sh, &acc);
    const double rzn = sh.out[0], beta = rzn / rz;
    for (int v = threadIdx.x; v < in.n; v += GBA_LANES) {
        if (D.fixed[v]) continue;
#pragma unroll
        for (int k = 0; k < 6; ++k) D.p[6 * v + k] = D.z[6 * v + k] + beta * D.p[6 * v + k];
    }
    if (threadIdx.x != 0) return;
    rec->rz = rzn; rec->cg_it = it + 1;
    if (rzn <= stop) { rec->cg_done = 1; rec->cg_total += it + 1; }
    else if (it + 1 >= in.cg_cap) { rec->cg_done = 1; rec->cg_total += it + 1; ++rec->cg_capped; }
}

// ---- the trial state and the decision -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void gba_ph_point_update(const GbaDev &D)
{
    __shared__ GbaRed<1> sh;
    const GbaRec *rec = D.rec;
    if (!(gba_in_tail(rec) && rec->trial_ok)) return;
    const GbaIn &in = *D.in;
    const size_t L = (size_t)in.nl;
    const double lambda = rec->lambda;
    double acc = 0.0;
    for (int j = 0; j < GBA_CHUNK / GBA_LANES; ++j) {
        const int l = blockIdx.x * GBA_CHUNK + j * GBA_LANES + threadIdx.x;
        if (l >= in.nl) break;
        double s[3], t[3], dl[3], bl[3], Hi[6], X[3];
        gba_point_gather(D, D.x, l, (size_t)in.ne, s);
#pragma unroll
        for (int k = 0; k < 6; ++k) Hi[k] = D.Hinv[k * L + l];
#pragma unroll
        for (int c = 0; c < 3; ++c) { bl[c] = D.bl[c * L + l]; t[c] = bl[c] - s[c]; X[c] = D.X[3 * (size_t)l + c]; }
        gb_sym3_mul(Hi, t, dl);
        const int zero = dl[0] == 0.0 && dl[1] == 0.0 && dl[2] == 0.0;
        double term = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            D.Xn[3 * (size_t)l + c] = zero ? X[c] : X[c] + dl[c];
            term += dl[c] * (lambda * dl[c] + bl[c]);
        }
        acc += term;
    }
    gba_reduce<1>(sh, &acc);
    if (threadIdx.x == 0) D.lpart[blockIdx.x] = sh.out[0];
}

__device__ __forceinline__ void gba_ph_pose_update(const GbaDev &D)
{
    const GbaRec *rec = D.rec;
    if (!(gba_in_tail(rec) && rec->trial_ok)) return;
    const GbaIn &in = *D.in;
    const int v = blockIdx.x * GBA_LANES + threadIdx.x;
    if (v >= in.n) return;
    const double lambda = rec->lambda;
    double T[7], Tn[7], x[6], acc = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) T[k] = D.T[7 * v + k];
    int zero = 1;
    const int fx = D.fixed[v];
    if (!fx)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            x[k] = D.x[6 * v + k];
            zero &= x[k] == 0.0;
            acc += x[k] * (lambda * x[k] + D.bp[6 * v + k]);
        }
    if (fx || zero) {
#pragma unroll
        for (int k = 0; k < 7; ++k) Tn[k] = T[k];
    } else {
        ygz_se3_retract(T, x, Tn);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) D.Tn[7 * v + k] = Tn[k];
    D.sterm[v] = acc;
}

__device__ __forceinline__ void gba_ph_decide(const GbaDev &D)
{
    __shared__ GbaRed<1> sh;
    GbaRec *rec = D.rec;
    if (!gba_in_tail(rec)) return;
    const GbaIn &in = *D.in;
    int ok = rec->trial_ok;
    const int bad_cost = rec->bad_cost;
    double tempChi = GB_DMAX, scale = 0.0;
    if (ok) {
        const double sp = gba_sum1(sh, D.sterm, in.n);
        const double sl = gba_sum1(sh, D.lpart, (in.nl + GBA_CHUNK - 1) / GBA_CHUNK);
        scale = sp + sl;
        tempChi = gba_sum1(sh, D.cpart, (in.ne + GBA_CHUNK - 1) / GBA_CHUNK);
        ok = !bad_cost && fabs(tempChi) <= GB_DMAX;
        if (!ok) { tempChi = GB_DMAX; scale = 0.0; }
    }
    if (threadIdx.x != 0) return;
    rec->bad_cost = 0;
    double lambda = rec->lambda, ni = rec->ni, currentChi = rec->currentChi;
    int qmax = rec->qmax, finished = 0, status = rec->status, accepted = 0, end_iteration = 0;
    scale += 1e-3;
    double rho = (currentChi - tempChi) / scale;
    if (!(fabs(rho) <= GB_DMAX)) rho = -1.0;
    int converged = 0;
    if (ok && rho > 0) {
        const double u = 2.0 * rho - 1.0;
        double alpha = 1.0 - u * u * u;
        if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
        lambda = lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
        ni = 2.0;
        converged = currentChi - tempChi <= in.min_rel_decrease * currentChi;
        currentChi = tempChi;
        accepted = 1;
        ++qmax;
        end_iteration = 1;
    } else {
        lambda = lambda * ni; ni = ni * 2.0;
        if (!(fabs(lambda) <= GB_DMAX)) end_iteration = 1;
        else {
            ++qmax;
            end_iteration = !(rho < 0 && qmax < in.max_trials);
        }
    }
    if (end_iteration) {
        ++rec->lm_iterations;
        if (qmax == in.max_trials || rho == 0 || !(fabs(lambda) <= GB_DMAX)) { status = YGZ_GBA_STALLED; finished = 1; }
        else if (converged) { status = YGZ_GBA_CONVERGED; finished = 1; }
        else if (rec->lm_iterations >= in.max_iterations) finished = 1;
        qmax = 0;
    }
    rec->lambda = lambda; rec->ni = ni; rec->currentChi = currentChi; rec->tempChi = tempChi; rec->rho = rho;
    rec->qmax = qmax; rec->status = status; rec->converged = converged;
    rec->accepted = accepted; rec->finished = finished; rec->decided = 1;
}

__device__ __forceinline__ void gba_ph_accept(const GbaDev &D)
{
    const GbaRec *rec = D.rec;
    if (!(rec->decided && rec->accepted)) return;
    const GbaIn &in = *D.in;
    const size_t nT = 7 * (size_t)in.n, nX = 3 * (size_t)in.nl;
    for (size_t k = (size_t)blockIdx.x * GBA_LANES + threadIdx.x; k < nT + nX; k += (size_t)gridDim.x * GBA_LANES) {
        if (k < nT) D.T[k] = D.Tn[k];
        else D.X[k - nT] = D.Xn[k - nT];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
bool finite_n(const double *v, size_t n)
{
    for (size_t k = 0; k < n; ++k) if (!(std::fabs(v[k]) <= GB_DMAX)) return false;
    return true;
}

// the device block.  Per edge (rows = 3, sba.hip): 61 bytes of upload (two indices, three observation doubles, kind, level, six CSR
// entries), 536 of work (res 24, w 8, Jp 144, Jl 72, Hpl 144 in each of the two slot orders) and 9 of classification (flag, chi2): 606 B.
// With rows = 2 (gba.hip): 48 + 456 = 504 B.  Everything else is per pose, per point or per chunk of GBA_CHUNK edges
struct Layout {
    size_t in, rec, fixed, edge_pose, edge_point, obs, kind, level, pt_off, pt_adj, pt_pose, ps_off, ps_adj, ps_point, slot_l, slot_p, t, x, in_end;   // the upload
    size_t tn, xn, res, w, jp, jl, hplp, hpll, cpart, lpart, hpp, bp, pose_vec, vterm, sterm, hll, bl, hinv, wl, vl, outlier, chi2, ipart, total;      // work
};
Layout layout(size_t N, size_t L, size_t E, size_t rows)
{
    const bool sba = rows == 3;
    Layout Y;
    YgzBlobLayout B;
    Y.in = B.add(sizeof(GbaIn));
    Y.rec = B.add(sizeof(GbaRec));
    Y.fixed = B.add(N);
    Y.edge_pose = B.add_n<int32_t>(E);
    Y.edge_point = B.add_n<int32_t>(E);
    Y.obs = B.add_n<double>(E * rows);
    Y.kind = B.add(sba ? E : 0);
    Y.level = B.add_n<int32_t>(sba ? E : 0);
    Y.pt_off = B.add_n<int32_t>(L + 1);
    Y.pt_adj = B.add_n<int32_t>(E);
    Y.pt_pose = B.add_n<int32_t>(E);
    Y.ps_off = B.add_n<int32_t>(N + 1);
    Y.ps_adj = B.add_n<int32_t>(E);
    Y.ps_point = B.add_n<int32_t>(E);
    Y.slot_l = B.add_n<int32_t>(E);
    Y.slot_p = B.add_n<int32_t>(E);
    Y.t = B.add_n<double>(N * 7);
    Y.x = B.add_n<double>(L * 3);
    Y.in_end = B.end;
    Y.tn = B.add_n<double>(N * 7);
    Y.xn = B.add_n<double>(L * 3);
    Y.res = B.add_n<double>(E * rows);
    Y.w = B.add_n<double>(E);
    Y.jp = B.add_n<double>(E * 6 * rows);
    Y.jl = B.add_n<double>(E * 3 * rows);
    Y.hplp = B.add_n<double>(E * 18);
    Y.hpll = B.add_n<double>(E * 18);
    Y.cpart = B.add_n<double>((E + GBA_CHUNK - 1) / GBA_CHUNK);
    Y.lpart = B.add_n<double>((L + GBA_CHUNK - 1) / GBA_CHUNK);
    Y.hpp = B.add_n<double>(N * 21);
    Y.bp = B.add_n<double>(N * 6);
    Y.pose_vec = B.add(ygz_round_up_256(N * 168) + 6 * ygz_round_up_256(N * 48));         // Lf, then bt x r z p q
    Y.vterm = B.add_n<double>(N);
    Y.sterm = B.add_n<double>(N);
    Y.hll = B.add_n<double>(L * 6);
    Y.bl = B.add_n<double>(L * 3);
    Y.hinv = B.add_n<double>(L * 6);
    Y.wl = B.add_n<double>(L * 3);
    Y.vl = B.add_n<double>(L * 3);
    Y.outlier = B.add(sba ? E : 0);
    Y.chi2 = B.add_n<double>(sba ? E : 0);
    Y.ipart = B.add_n<int32_t>(sba ? (E + GBA_CHUNK - 1) / GBA_CHUNK : 0);
    Y.total = B.end;
    return Y;
}

// the CSR list of key [E] over n_keys keys (gb_csr), and every edge's position in it
void csr(int n_keys, int ne, const int32_t *key, int32_t *off, int32_t *adj, int32_t *slot)
{
    for (int v = 0; v <= n_keys; ++v) off[v] = 0;
    for (int e = 0; e < ne; ++e) ++off[key[e] + 1];
    for (int v = 0; v < n_keys; ++v) off[v + 1] += off[v];
    std::vector<int32_t> fill(off, off + n_keys);
    for (int e = 0; e < ne; ++e) { const int s = fill[key[e]]++; adj[s] = e; slot[e] = s; }
}

// a validated problem as both entry points hand it to the driver; rows: residual rows per edge (2: gba.hip, 3: sba.hip with kind and level)
struct GbaProblem {
    int n, nl, ne, rows;
    const double *poses, *points, *obs, *K4;
    const uint8_t *fixed;
    const int32_t *edge_pose, *edge_point;
    const uint8_t *kind;
    const int32_t *level;
};

// the fifteen kernels of one edge model: every file wraps the shared phase bodies in kernels of its own
struct GbaKernels {
    void (*linearize)(GbaDev, int);
    void (*point_system)(GbaDev, int);
    void (*pose_system)(GbaDev, int);
    void (*begin)(GbaDev);
    void (*point_trial)(GbaDev);
    void (*pose_trial)(GbaDev);
    void (*cg_begin)(GbaDev);
    void (*cg_point)(GbaDev);
    void (*cg_pose)(GbaDev);
    void (*cg_step)(GbaDev);
    void (*point_update)(GbaDev);
    void (*pose_update)(GbaDev);
    void (*cost)(GbaDev);
    void (*decide)(GbaDev);
    void (*accept)(GbaDev);
};

struct Run {
    uint8_t *dev, *host;                      // the device block and the page-locked area the results come back into
    uint8_t *up;                              // the page-locked image of the upload
    Layout Y;
    GbaDev D;
    GbaIn in;
    GbaRec rec;                               // the control record as last read back
    size_t N, L, E;
    long launches;                            // kernels queued so far
};

// the CSR lists, one upload, the device pointers, the clears.  `in` is complete but for n, nl, ne, K and cg_cap (cg_max_iterations <= 0:
// the automatic cap); down_bytes: the page-locked area behind the upload's image that the results come back into
int gba_open(ygz_hip_ctx *ctx, int scratch_id, const GbaProblem &pb, GbaIn in, int cg_max_iterations, size_t down_bytes, Run *R)
{
    const int n = pb.n, nl = pb.nl, ne = pb.ne;
    const size_t N = (size_t)n, L = (size_t)nl, E = (size_t)ne, rows = (size_t)pb.rows;
    const Layout Y = layout(N, L, E, rows);
    YgzBlob blob;
    int rc = ygz_blob_open(ctx, scratch_id, Y.total, Y.in_end + down_bytes, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = blob.host, *dev = blob.dev;
    int n_free = 0;
    for (int v = 0; v < n; ++v) n_free += !pb.fixed[v];
    for (int k = 0; k < 4; ++k) in.K[k] = pb.K4[k];
    in.n = n; in.nl = nl; in.ne = ne;
    in.cg_cap = cg_max_iterations > 0 ? cg_max_iterations : (6 * n_free < GBA_CG_CAP ? 6 * n_free : GBA_CG_CAP);
    memcpy(up + Y.in, &in, sizeof in);
    memset(up + Y.rec, 0, sizeof(GbaRec));
    for (int v = 0; v < n; ++v) up[Y.fixed + v] = pb.fixed[v] ? 1 : 0;
    memcpy(up + Y.edge_pose, pb.edge_pose, E * 4);
    memcpy(up + Y.edge_point, pb.edge_point, E * 4);
    memcpy(up + Y.obs, pb.obs, E * rows * 8);
    if (pb.rows == 3) { memcpy(up + Y.kind, pb.kind, E); memcpy(up + Y.level, pb.level, E * 4); }
    memcpy(up + Y.t, pb.poses, N * 56);
    memcpy(up + Y.x, pb.points, L * 24);
    int32_t *pt_adj = (int32_t *)(up + Y.pt_adj), *pt_pose = (int32_t *)(up + Y.pt_pose), *ps_adj = (int32_t *)(up + Y.ps_adj),
            *ps_point = (int32_t *)(up + Y.ps_point);
    csr(nl, ne, pb.edge_point, (int32_t *)(up + Y.pt_off), pt_adj, (int32_t *)(up + Y.slot_l));
    csr(n, ne, pb.edge_pose, (int32_t *)(up + Y.ps_off), ps_adj, (int32_t *)(up + Y.slot_p));
    for (int s = 0; s < ne; ++s) {
        const int v = pb.edge_pose[pt_adj[s]];
        pt_pose[s] = pb.fixed[v] ? -1 : v;
        ps_point[s] = pb.edge_point[ps_adj[s]];
    }
    if ((rc = ygz_blob_upload(ctx, blob, Y.in_end)) != YGZ_OK) return rc;
    GbaDev D;
    D.in = (const GbaIn *)(dev + Y.in); D.rec = (GbaRec *)(dev + Y.rec); D.fixed = dev + Y.fixed;
    D.edge_pose = (const int32_t *)(dev + Y.edge_pose); D.edge_point = (const int32_t *)(dev + Y.edge_point); D.obs = (const double *)(dev + Y.obs);
    D.kind = dev + Y.kind; D.level = (const int32_t *)(dev + Y.level); D.outlier = dev + Y.outlier; D.chi2 = (double *)(dev + Y.chi2);
    D.ipart = (int32_t *)(dev + Y.ipart);
    D.pt_off = (const int32_t *)(dev + Y.pt_off); D.pt_adj = (const int32_t *)(dev + Y.pt_adj); D.pt_pose = (const int32_t *)(dev + Y.pt_pose);
    D.ps_off = (const int32_t *)(dev + Y.ps_off); D.ps_adj = (const int32_t *)(dev + Y.ps_adj); D.ps_point = (const int32_t *)(dev + Y.ps_point);
    D.slot_l = (const int32_t *)(dev + Y.slot_l); D.slot_p = (const int32_t *)(dev + Y.slot_p);
    D.T = (double *)(dev + Y.t); D.X = (double *)(dev + Y.x); D.Tn = (double *)(dev + Y.tn); D.Xn = (double *)(dev + Y.xn);
    D.res = (double *)(dev + Y.res); D.w = (double *)(dev + Y.w); D.Jp = (double *)(dev + Y.jp); D.Jl = (double *)(dev + Y.jl);
    D.HplP = (double *)(dev + Y.hplp); D.HplL = (double *)(dev + Y.hpll); D.cpart = (double *)(dev + Y.cpart); D.lpart = (double *)(dev + Y.lpart);
    D.Hpp = (double *)(dev + Y.hpp); D.bp = (double *)(dev + Y.bp);
    const size_t vs = ygz_round_up_256(N * 48);
    uint8_t *pv = dev + Y.pose_vec;
    D.Lf = (double *)pv; pv += ygz_round_up_256(N * 168);
    D.bt = (double *)pv; D.x = (double *)(pv + vs); D.r = (double *)(pv + 2 * vs); D.z = (double *)(pv + 3 * vs); D.p = (double *)(pv + 4 * vs);
    D.q = (double *)(pv + 5 * vs);
    D.vterm = (double *)(dev + Y.vterm); D.sterm = (double *)(dev + Y.sterm);
    D.Hll = (double *)(dev + Y.hll); D.bl = (double *)(dev + Y.bl); D.Hinv = (double *)(dev + Y.hinv); D.wl = (double *)(dev + Y.wl);
    D.vl = (double *)(dev + Y.vl);
    // Hpp and bp of the fixed poses are never written: the stage export shows zeros; vterm of the fixed poses stays zero in every sum
    YGZ_HIPCHK(ctx, hipMemsetAsync(dev + Y.hpp, 0, Y.pose_vec - Y.hpp, ctx->stream));
    YGZ_HIPCHK(ctx, hipMemsetAsync(dev + Y.vterm, 0, Y.hll - Y.vterm, ctx->stream));
    R->dev = dev; R->up = up; R->host = up + Y.in_end; R->Y = Y; R->D = D; R->in = in; R->N = N; R->L = L; R->E = E; R->launches = 0;
    memset(&R->rec, 0, sizeof R->rec);
    return YGZ_OK;
}

// the linearisation at the estimate, ungated: residuals, blocks, the system, the cost, lambda_0 and the record
int gba_linearize_first(ygz_hip_ctx *ctx, const GbaKernels &K, Run *R)
{
    const GbaDev &D = R->D;
    const dim3 blk(GBA_LANES);
    const dim3 g_edges((unsigned)((R->E + GBA_CHUNK - 1) / GBA_CHUNK)), g_points((unsigned)((R->L + GBA_LANES - 1) / GBA_LANES)), g_poses((unsigned)R->N), one(1);
    YGZ_LAUNCH(ctx, KID_COUNT, K.linearize, g_edges, blk, D, 0);
    YGZ_LAUNCH(ctx, KID_COUNT, K.point_system, g_points, blk, D, 0);
    YGZ_LAUNCH(ctx, KID_COUNT, K.pose_system, g_poses, blk, D, 0);
    YGZ_LAUNCH(ctx, KID_COUNT, K.begin, one, blk, D);
    R->launches += 4;
    YGZ_HIPCHK(ctx, hipGetLastError());
    return YGZ_OK;
}

// the stage export: the record and the eight arrays of the linearisation into the page-locked area, each at a multiple of 256 bytes; the wait
int gba_fetch_stage(ygz_hip_ctx *ctx, Run *R, size_t rows)
{
    const Layout &Y = R->Y;
    const size_t N = R->N, L = R->L, E = R->E;
    uint8_t *h = R->host;
    size_t o = 0;
    const struct { size_t src, bytes; } parts[] = { { Y.rec, sizeof(GbaRec) }, { Y.res, E * rows * 8 }, { Y.w, E * 8 }, { Y.jp, E * rows * 48 },
                                                    { Y.jl, E * rows * 24 }, { Y.hpp, N * 168 }, { Y.bp, N * 48 }, { Y.hll, L * 48 }, { Y.bl, L * 24 } };
    for (const auto &q : parts) {
        YGZ_HIPCHK(ctx, hipMemcpyAsync(h + o, R->dev + q.src, q.bytes, hipMemcpyDeviceToHost, ctx->stream));
        o += ygz_round_up_256(q.bytes);
    }
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    R->rec = *(const GbaRec *)h;
    return YGZ_OK;
}

// the LM loop behind gba_linearize_first: trials of lambda, CG iterations queued in batches with one small read-back per batch, until the
// record says finished.  Afterwards the device block holds the estimate and R->rec the record
int gba_solve(ygz_hip_ctx *ctx, const GbaKernels &K, Run *R, int max_iterations, int max_trials, int cg_batch)
{
    const GbaDev &D = R->D;
    const size_t N = R->N, L = R->L, E = R->E;
    const dim3 blk(GBA_LANES);
    const dim3 g_edges((unsigned)((E + GBA_CHUNK - 1) / GBA_CHUNK)), g_points((unsigned)((L + GBA_LANES - 1) / GBA_LANES)), g_poses((unsigned)N),
               g_pchunks((unsigned)((L + GBA_CHUNK - 1) / GBA_CHUNK)), g_pose_lanes((unsigned)((N + GBA_LANES - 1) / GBA_LANES)), one(1);
    const size_t n_copy = 7 * N + 3 * L;
    const dim3 g_copy((unsigned)std::min<size_t>((n_copy + GBA_LANES - 1) / GBA_LANES, 1024));
    GbaRec *hrec = (GbaRec *)R->host;
    YGZ_HIPCHK(ctx, hipMemcpyAsync(hrec, D.rec, sizeof(GbaRec), hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int batch = cg_batch > 0 ? cg_batch : GBA_DEFAULT_BATCH;
    const int max_batches = (R->in.cg_cap + batch - 1) / batch + 1;
    // at most max_iterations x max_trials trials, each of at most max_batches batches: the number of launches is bounded by the caps
    for (long trial = 0; !hrec->finished && trial < (long)max_iterations * max_trials; ++trial) {
        YGZ_LAUNCH(ctx, KID_COUNT, K.point_trial, g_points, blk, D);
        YGZ_LAUNCH(ctx, KID_COUNT, K.pose_trial, g_poses, blk, D);
        YGZ_LAUNCH(ctx, KID_COUNT, K.cg_begin, one, blk, D);
        R->launches += 3;
        int b = 0;
        for (; b < max_batches; ++b) {
            for (int it = 0; it < batch; ++it) {
                YGZ_LAUNCH(ctx, KID_COUNT, K.cg_point, g_points, blk, D);
                YGZ_LAUNCH(ctx, KID_COUNT, K.cg_pose, g_poses, blk, D);
                YGZ_LAUNCH(ctx, KID_COUNT, K.cg_step, one, blk, D);
            }
            // the tail runs once the solve has ended, whichever batch that is; behind an unfinished solve every kernel of it returns at once
            YGZ_LAUNCH(ctx, KID_COUNT, K.point_update, g_pchunks, blk, D);
            YGZ_LAUNCH(ctx, KID_COUNT, K.pose_update, g_pose_lanes, blk, D);
            YGZ_LAUNCH(ctx, KID_COUNT, K.cost, g_edges, blk, D);
            YGZ_LAUNCH(ctx, KID_COUNT, K.decide, one, blk, D);
            YGZ_LAUNCH(ctx, KID_COUNT, K.accept, g_copy, blk, D);
            YGZ_LAUNCH(ctx, KID_COUNT, K.linearize, g_edges, blk, D, 1);
            YGZ_LAUNCH(ctx, KID_COUNT, K.point_system, g_points, blk, D, 1);
            YGZ_LAUNCH(ctx, KID_COUNT, K.pose_system, g_poses, blk, D, 1);
            R->launches += 3 * (long)batch + 8;
            YGZ_HIPCHK(ctx, hipGetLastError());
            YGZ_HIPCHK(ctx, hipMemcpyAsync(hrec, D.rec, sizeof(GbaRec), hipMemcpyDeviceToHost, ctx->stream));
            YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            if (hrec->decided) break;
        }
        if (b == max_batches) return YGZ_E_STATE;                      // cannot happen: the cap ends the solve within max_batches
    }
    R->rec = *hrec;
    return YGZ_OK;
}

// [K][n] -> [n][K]
void to_rows(const double *soa, size_t n, int K, double *rows)
{
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < K; ++k) rows[i * K + k] = soa[(size_t)k * n + i];
}

}  // namespace
