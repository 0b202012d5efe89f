// Stereo bundle adjustment (ORB-SLAM2's Optimizer::LocalBundleAdjustment / GlobalBundleAdjustemnt with stereo edges; nothing in the reference):
// keyframe poses and map points against mono (u, v) and stereo (u, v, uR) observations, the information scaled by the pyramid level, g2o's
// Huber kernel on chi2, rounds of Levenberg-Marquardt with every edge classified in between and the outliers switched off.  The solver is
// gba.hip's -- the Schur-complement PCG of gba_phases.h, whose eleven edge-agnostic phases and host driver are shared, not copied; this
// file holds the edge model (four kernels) and the classification.  The arithmetic is tests/sba_ref.c's decision by decision
// (-ffp-contract=off, only + - * / and sqrt), so every output is bit-identical to it.
//   k_sba_linearize      lane = edge (GBA_CHUNK per workgroup): res [3][E], weight, Jp [18][E], Jl [9][E], Hpl in both CSR orders, cost chunk sums;
//                        an absent or inactive edge writes exact zeros into all of them and is never tested
//   k_sba_point_system   lane = point: Hll, bl over the point's edges, three-row sums
//   k_sba_pose_system    workgroup = pose: Hpp, bp lane-strided over the pose's edges (three-row sums, still 27 quantities), then the tree
//   k_sba_cost           lane = edge: the robust cost of the trial state over the active edges
//   k_sba_classify       lane = 4 edges: every present edge at the estimate without kernel: outlier, chi2, the chunk's inlier count
//   k_sba_begin .. k_sba_accept: the eleven bodies of gba_phases.h
// Per edge the device block holds 606 bytes (gba_phases.h, Layout).
#pragma clang fp contract(off)
#define GBA_LANES 256                      // GB_LANES of tests/gba_ref.c: the lanes of the fixed summation order
#define GBA_CHUNK 1024                     // GB_CHUNK: elements per first-level chunk of a two-level sum
#define GBA_CG_CAP 1024                    // GB_CG_CAP: bound of the automatic CG cap
#include "gba_phases.h"

namespace {

// ---- one edge (tests/sba_ref.c, function by function; its level weight is ygz_level_weight of posemath_dev.h) ---------------------------
__device__ __forceinline__ int sb_residual(const double *T, const double *X, const double *ob, const double *K, double bf, int kind, double *R,
                                           double *P, double *r)
{
    r[2] = 0.0;
    if (!gb_residual(T, X, ob, K, R, P, r)) return 0;
    if (kind != 2) return 1;
    r[2] = ob[2] - ((K[0] * (P[0] / P[2]) + K[2]) - bf / P[2]);
    return fabs(r[2]) <= GB_DMAX;
}

__device__ __forceinline__ double sb_chi2(const double *r, int kind, double w)
{
    double e2 = r[0] * r[0] + r[1] * r[1];
    if (kind == 2) e2 = e2 + r[2] * r[2];
    return w * e2;
}

__device__ __forceinline__ void sb_robust(double chi2, int on, double d2, double delta, double *rho0, double *rho1)
{
    *rho0 = chi2; *rho1 = 1.0;
    if (on && chi2 > d2) {
        const double s = sqrt(chi2);
        *rho0 = 2.0 * s * delta - d2;
        *rho1 = delta / s;
    }
}

__device__ __forceinline__ int sb_edge_terms(const double *T, const double *X, const double *ob, const double *K, double bf, int kind, int level,
                                             int robust, double d2, double delta, double *r, double *wgt, double *rho, double *Jp, double *Jl)
{
    double R[9], P[3], w0, rho0;
    int ok = gb_edge_terms(T, X, ob, K, 0.0, r, &w0, &rho0, Jp, Jl);
    r[2] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) Jp[12 + k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) Jl[6 + k] = 0.0;
    if (ok) ok = sb_residual(T, X, ob, K, bf, kind, R, P, r);
    if (!ok) {
        r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; *wgt = 0.0; *rho = 0.0;
#pragma unroll
        for (int k = 0; k < 18; ++k) Jp[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) Jl[k] = 0.0;
        return 0;
    }
    if (kind == 2) {
        const double x = P[0], y = P[1], z = P[2], e = (bf / z) / z;
        Jp[12] = Jp[0] - e * y; Jp[13] = Jp[1] + e * x; Jp[14] = Jp[2]; Jp[15] = Jp[3]; Jp[16] = Jp[4]; Jp[17] = Jp[5] - e;
#pragma unroll
        for (int k = 0; k < 3; ++k) Jl[6 + k] = Jl[k] - e * R[6 + k];
    }
    const double w = ygz_level_weight(level);
    double rho1;
    sb_robust(sb_chi2(r, kind, w), robust, d2, delta, rho, &rho1);
    *wgt = rho1 * w;
    return 1;
}

__device__ __forceinline__ bool sb_active(const GbaDev &D, const GbaIn &in, int e, int *kind)
{
    *kind = D.kind[e];
    return *kind != 0 && !(in.use_outliers && D.outlier[e]);
}

// ---- the four phases that see the edge model -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBA_LANES) void k_sba_linearize(GbaDev D, int gated)
{
    __shared__ GbaRed<1> sh;
    if (gated && !gba_after_accept(D.rec)) return;
    const GbaIn &in = *D.in;
    const size_t E = (size_t)in.ne;
    const double K[4] = { in.K[0], in.K[1], in.K[2], in.K[3] };
    int bad = 0;
    double acc = 0.0;
    for (int j = 0; j < GBA_CHUNK / GBA_LANES; ++j) {
        const int e = blockIdx.x * GBA_CHUNK + j * GBA_LANES + threadIdx.x;
        if (e >= in.ne) break;
        double r[3] = { 0.0, 0.0, 0.0 }, w = 0.0, rho = 0.0, Jp[18], Jl[9];
#pragma unroll
        for (int k = 0; k < 18; ++k) Jp[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) Jl[k] = 0.0;
        int kind;
        const bool active = sb_active(D, in, e, &kind);
        if (active) {
            const int v = D.edge_pose[e], l = D.edge_point[e];
            double T[7], X[3], ob[3];
#pragma unroll
            for (int k = 0; k < 7; ++k) T[k] = D.T[7 * v + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) { X[k] = D.X[3 * (size_t)l + k]; ob[k] = D.obs[3 * (size_t)e + k]; }
            bad |= !sb_edge_terms(T, X, ob, K, in.bf, kind, D.level[e], in.robust, kind == 2 ? in.d2s : in.d2m, kind == 2 ? in.ds : in.dm, r, &w, &rho,
                                  Jp, Jl);
        }
        acc += rho;
#pragma unroll
        for (int k = 0; k < 3; ++k) D.res[k * E + e] = r[k];
        D.w[e] = w;
#pragma unroll
        for (int k = 0; k < 18; ++k) D.Jp[k * E + e] = Jp[k];
#pragma unroll
        for (int k = 0; k < 9; ++k) D.Jl[k * E + e] = Jl[k];
        const size_t sp = (size_t)D.slot_p[e], sl = (size_t)D.slot_l[e];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const double two = Jp[a] * Jl[b] + Jp[6 + a] * Jl[3 + b];
                const double h = kind == 2 ? w * (two + Jp[12 + a] * Jl[6 + b]) : w * two;
                D.HplP[(3 * a + b) * E + sp] = h;
                D.HplL[(3 * a + b) * E + sl] = h;
            }
    }
    gba_reduce<1>(sh, &acc);
    if (threadIdx.x == 0) D.cpart[blockIdx.x] = sh.out[0];
    if (bad) atomicOr(&D.rec->bad_lin, 1);
}

// the third row's products are +0.0 for a mono, an absent and an inactive edge: no bit of a sum that starts at +0.0 changes
__global__ __launch_bounds__(GBA_LANES) void k_sba_point_system(GbaDev D, int gated)
{
    if (gated && !gba_after_accept(D.rec)) return;
    const GbaIn &in = *D.in;
    const size_t E = (size_t)in.ne, L = (size_t)in.nl;
    const int l = blockIdx.x * GBA_LANES + threadIdx.x;
    if (l >= in.nl) return;
    double h[6], g[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) h[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = 0.0;
    for (int s = D.pt_off[l]; s < D.pt_off[l + 1]; ++s) {
        const size_t e = (size_t)D.pt_adj[s];
        double J[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) J[k] = D.Jl[k * E + e];
        const double r0 = D.res[e], r1 = D.res[E + e], r2 = D.res[2 * E + e], w = D.w[e];
        int m = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a; b < 3; ++b) h[m++] += w * ((J[a] * J[b] + J[3 + a] * J[3 + b]) + J[6 + a] * J[6 + b]);
            g[a] += w * ((J[a] * r0 + J[3 + a] * r1) + J[6 + a] * r2);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) D.Hll[k * L + l] = h[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) D.bl[k * L + l] = -g[k];
    gba_max_diag(D.rec, h[0]); gba_max_diag(D.rec, h[3]); gba_max_diag(D.rec, h[5]);
}

__global__ __launch_bounds__(GBA_LANES) void k_sba_pose_system(GbaDev D, int gated)
{
    __shared__ GbaRed<27> sh;
    if (gated && !gba_after_accept(D.rec)) return;
    const int v = blockIdx.x;
    if (D.fixed[v]) return;
    const size_t E = (size_t)D.in->ne;
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int s = D.ps_off[v] + threadIdx.x; s < D.ps_off[v + 1]; s += GBA_LANES) {
        const size_t e = (size_t)D.ps_adj[s];
        double J[18];
#pragma unroll
        for (int k = 0; k < 18; ++k) J[k] = D.Jp[k * E + e];
        const double r0 = D.res[e], r1 = D.res[E + e], r2 = D.res[2 * E + e], w = D.w[e];
        int m = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) acc[m++] += w * ((J[a] * J[b] + J[6 + a] * J[6 + b]) + J[12 + a] * J[12 + b]);
            acc[21 + a] += w * ((J[a] * r0 + J[6 + a] * r1) + J[12 + a] * r2);
        }
    }
    gba_reduce<27>(sh, acc);
    const int tid = threadIdx.x;
    if (tid < 21) D.Hpp[21 * v + tid] = sh.out[tid];
    else if (tid < 27) D.bp[6 * v + tid - 21] = -sh.out[tid];
    if (tid == 0) {
        int m = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) { gba_max_diag(D.rec, sh.out[m]); m += 6 - a; }
    }
}

__global__ __launch_bounds__(GBA_LANES) void k_sba_cost(GbaDev D)
{
    __shared__ GbaRed<1> sh;
    const GbaRec *rec = D.rec;
    if (!(gba_in_tail(rec) && rec->trial_ok)) return;
    const GbaIn &in = *D.in;
    const double K[4] = { in.K[0], in.K[1], in.K[2], in.K[3] };
    int bad = 0;
    double acc = 0.0;
    for (int j = 0; j < GBA_CHUNK / GBA_LANES; ++j) {
        const int e = blockIdx.x * GBA_CHUNK + j * GBA_LANES + threadIdx.x;
        if (e >= in.ne) break;
        int kind;
        double term = 0.0;
        if (sb_active(D, in, e, &kind)) {
            const int v = D.edge_pose[e], l = D.edge_point[e];
            double T[7], X[3], ob[3], R[9], P[3], r[3], rho1;
#pragma unroll
            for (int k = 0; k < 7; ++k) T[k] = D.Tn[7 * v + k];
#pragma unroll
            for (int k = 0; k < 3; ++k) { X[k] = D.Xn[3 * (size_t)l + k]; ob[k] = D.obs[3 * (size_t)e + k]; }
            if (!sb_residual(T, X, ob, K, in.bf, kind, R, P, r)) bad = 1;
            else sb_robust(sb_chi2(r, kind, ygz_level_weight(D.level[e])), in.robust, kind == 2 ? in.d2s : in.d2m, kind == 2 ? in.ds : in.dm, &term, &rho1);
        }
        acc += term;
    }
    gba_reduce<1>(sh, &acc);
    if (threadIdx.x == 0) D.cpart[blockIdx.x] = sh.out[0];
    if (bad) atomicOr(&D.rec->bad_cost, 1);
}

// every present edge at the estimate by a fresh evaluation without kernel.  The inlier count of the chunk goes to ipart [chunk]: lane sums,
// the wavefront's by shuffles, the four wavefronts' by lane 0; integers, so the order is free.  The host adds the chunks
__global__ __launch_bounds__(GBA_LANES) void k_sba_classify(GbaDev D)
{
    __shared__ int32_t sh[GBA_LANES / 64];
    const GbaIn &in = *D.in;
    const double K[4] = { in.K[0], in.K[1], in.K[2], in.K[3] };
    int count = 0;
    for (int j = 0; j < GBA_CHUNK / GBA_LANES; ++j) {
        const int e = blockIdx.x * GBA_CHUNK + j * GBA_LANES + threadIdx.x;
        if (e >= in.ne) break;
        const int kind = D.kind[e];
        if (kind == 0) { D.outlier[e] = 0; D.chi2[e] = -1.0; continue; }
        const int v = D.edge_pose[e], l = D.edge_point[e];
        double T[7], X[3], ob[3], R[9], P[3], r[3];
#pragma unroll
        for (int k = 0; k < 7; ++k) T[k] = D.T[7 * v + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { X[k] = D.X[3 * (size_t)l + k]; ob[k] = D.obs[3 * (size_t)e + k]; }
        if (!sb_residual(T, X, ob, K, in.bf, kind, R, P, r)) { D.outlier[e] = 1; D.chi2[e] = 0.0; continue; }
        const double c = sb_chi2(r, kind, ygz_level_weight(D.level[e]));
        const int out = c > (kind == 2 ? in.d2s : in.d2m);
        D.outlier[e] = (uint8_t)out; D.chi2[e] = c;
        count += !out;
    }
#pragma unroll
    for (int st = 32; st >= 1; st >>= 1) count += __shfl_down(count, st);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) D.ipart[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---- the other eleven: gba_phases.h ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBA_LANES) void k_sba_begin(GbaDev D) { gba_ph_begin(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_point_trial(GbaDev D) { gba_ph_point_trial(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_pose_trial(GbaDev D) { gba_ph_pose_trial(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_cg_begin(GbaDev D) { gba_ph_cg_begin(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_cg_point(GbaDev D) { gba_ph_cg_point(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_cg_pose(GbaDev D) { gba_ph_cg_pose(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_cg_step(GbaDev D) { gba_ph_cg_step(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_point_update(GbaDev D) { gba_ph_point_update(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_pose_update(GbaDev D) { gba_ph_pose_update(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_decide(GbaDev D) { gba_ph_decide(D); }
__global__ __launch_bounds__(GBA_LANES) void k_sba_accept(GbaDev D) { gba_ph_accept(D); }

const GbaKernels KERNELS = { k_sba_linearize, k_sba_point_system, k_sba_pose_system, k_sba_begin, k_sba_point_trial, k_sba_pose_trial, k_sba_cg_begin,
                             k_sba_cg_point, k_sba_cg_pose, k_sba_cg_step, k_sba_point_update, k_sba_pose_update, k_sba_cost, k_sba_decide,
                             k_sba_accept };

// ---- host side ----------------------------------------------------------------------------------------------------------------------
struct SbaArgs {
    int n; const double *poses; const uint8_t *fixed; int nl; const double *points; int ne; const int32_t *edge_pose, *edge_point;
    const double *obs; const uint8_t *kind; const int32_t *level; const double *K4;
};

// every refusal of the header, in its order, before anything touches the device
int validate(const ygz_hip_ctx *ctx, const SbaArgs &a, const ygz_sba_params &p)
{
    const int n = a.n, nl = a.nl, ne = a.ne;
    if (!a.poses || !a.fixed || !a.points || !a.edge_pose || !a.edge_point || !a.obs || !a.kind || !a.level || !a.K4) return YGZ_E_INVALID;
    if (n > YGZ_GBA_MAX_POSES || nl > YGZ_GBA_MAX_POINTS || ne > YGZ_GBA_MAX_EDGES) return YGZ_E_CAPACITY;
    if (n < 2 || nl < 1 || ne < 1) return YGZ_E_INVALID;
    if (p.max_iterations < 1 || p.max_iterations > 1000 || p.max_trials < 1 || p.max_trials > 100 || p.cg_max_iterations < 0
        || p.cg_max_iterations > 65536 || p.cg_batch < 0 || p.cg_batch > 1024 || !(p.cg_tol > 0 && p.cg_tol < 1)
        || !(p.min_rel_decrease >= 0 && p.min_rel_decrease < 1))
        return YGZ_E_INVALID;
    if (!(p.chi2_mono > 0) || !(p.chi2_stereo > 0) || !finite_n(&p.chi2_mono, 1) || !finite_n(&p.chi2_stereo, 1)) return YGZ_E_INVALID;
    if (p.rounds < 1 || p.rounds > YGZ_SBA_MAX_ROUNDS || p.robust_rounds < 0 || p.robust_rounds > YGZ_SBA_MAX_ROUNDS) return YGZ_E_INVALID;
    for (int k = 0; k < p.rounds; ++k) if (p.iterations[k] < 1 || p.iterations[k] > 1000) return YGZ_E_INVALID;
    if (!finite_n(a.K4, 4) || !(a.K4[0] > 0) || !(a.K4[1] > 0)) return YGZ_E_INVALID;
    std::vector<int32_t> deg_pose(n, 0), deg_point(nl, 0);
    bool stereo = false;
    for (int e = 0; e < ne; ++e) {
        const int v = a.edge_pose[e], l = a.edge_point[e];
        if (v < 0 || v >= n || l < 0 || l >= nl) return YGZ_E_INVALID;
        if (a.kind[e] > 2) return YGZ_E_INVALID;
        if (a.level[e] < 0 || a.level[e] > 15 || (ctx && a.level[e] >= ctx->prm.pyramid_levels)) return YGZ_E_INVALID;
        if (a.kind[e] == 0) continue;
        stereo |= a.kind[e] == 2;
        ++deg_pose[v]; ++deg_point[l];
    }
    for (int e = 0; e < ne; ++e)                                       // uR of a mono edge and all of an absent edge are never read
        if (a.kind[e] && !finite_n(a.obs + 3 * (size_t)e, a.kind[e] == 2 ? 3 : 2)) return YGZ_E_INVALID;
    if (!finite_n(a.poses, 7 * (size_t)n) || !finite_n(a.points, 3 * (size_t)nl)) return YGZ_E_INVALID;
    if (stereo && (!(p.baseline > 0) || !finite_n(&p.baseline, 1))) return YGZ_E_INVALID;
    int n_free = 0;
    for (int v = 0; v < n; ++v) {
        const double *q = a.poses + 7 * (size_t)v;
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0)) return YGZ_E_INVALID;
        if (a.fixed[v]) continue;
        ++n_free;
        if (!deg_pose[v]) return YGZ_E_INVALID;
    }
    if (n_free < 1) return YGZ_E_INVALID;
    for (int l = 0; l < nl; ++l) if (deg_point[l] < 2) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    return YGZ_OK;
}

// validation, the shared driver's upload, then the rounds: the record and the round's switches go up again, the LM loop runs from the
// estimate the device holds, the classification follows, and one small read-back brings the chunks' inlier counts.  stage: the
// linearisation at the input alone.  The block is SCR_SBA's: the call joins on entry and waits before it returns
int run(ygz_hip_ctx *ctx, const SbaArgs &a, const ygz_sba_params *params, bool stage, Run *R, ygz_sba_result *res)
{
    ygz_sba_params p;
    if (params) p = *params; else ygz_hip_default_sba_params(&p);
    const int rv = validate(ctx, a, p);
    if (rv != YGZ_OK) return rv;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    const size_t N = (size_t)a.n, L = (size_t)a.nl, E = (size_t)a.ne, NC = (E + GBA_CHUNK - 1) / GBA_CHUNK;
    YgzBlobLayout down;
    down.add(sizeof(GbaRec));
    if (stage) for (size_t bytes : { E * 24, E * 8, E * 144, E * 72, N * 168, N * 48, L * 48, L * 24 }) down.add(bytes);
    else for (size_t bytes : { NC * 4, N * 56, L * 24, E, E * 8 }) down.add(bytes);
    GbaIn in;
    memset(&in, 0, sizeof in);
    in.cg_tol = p.cg_tol; in.min_rel_decrease = p.min_rel_decrease; in.max_iterations = p.iterations[0]; in.max_trials = p.max_trials;
    in.stage_only = stage ? 1 : 0;
    in.bf = a.K4[0] * p.baseline; in.d2m = p.chi2_mono; in.d2s = p.chi2_stereo; in.dm = std::sqrt(p.chi2_mono); in.ds = std::sqrt(p.chi2_stereo);
    in.robust = p.robust_rounds > 0; in.use_outliers = 0;
    const GbaProblem pb = { a.n, a.nl, a.ne, 3, a.poses, a.points, a.obs, a.K4, a.fixed, a.edge_pose, a.edge_point, a.kind, a.level };
    int rc = gba_open(ctx, SCR_SBA, pb, in, p.cg_max_iterations, down.end, R);
    if (rc != YGZ_OK) return rc;
    if (stage) {
        if ((rc = gba_linearize_first(ctx, KERNELS, R)) != YGZ_OK) return rc;
        return gba_fetch_stage(ctx, R, 3);
    }
    const Layout &Y = R->Y;
    int32_t *hpart = (int32_t *)(R->host + ygz_round_up_256(sizeof(GbaRec)));
    memset(res, 0, sizeof *res);
    for (int k = 0; k < p.rounds; ++k) {
        if (k > 0) {                                                    // the record zero-filled, the round's switches: one small copy
            R->in.max_iterations = p.iterations[k]; R->in.robust = k < p.robust_rounds; R->in.use_outliers = 1;
            memcpy(R->up + Y.in, &R->in, sizeof(GbaIn));
            memset(R->up + Y.rec, 0, sizeof(GbaRec));
            YGZ_HIPCHK(ctx, hipMemcpyAsync(R->dev + Y.in, R->up + Y.in, Y.fixed - Y.in, hipMemcpyHostToDevice, ctx->stream));
        }
        if ((rc = gba_linearize_first(ctx, KERNELS, R)) != YGZ_OK) return rc;
        if ((rc = gba_solve(ctx, KERNELS, R, p.iterations[k], p.max_trials, p.cg_batch)) != YGZ_OK) return rc;
        YGZ_LAUNCH(ctx, KID_COUNT, k_sba_classify, dim3((unsigned)NC), dim3(GBA_LANES), R->D);
        ++R->launches;
        YGZ_HIPCHK(ctx, hipGetLastError());
        YGZ_HIPCHK(ctx, hipMemcpyAsync(hpart, R->dev + Y.ipart, NC * 4, hipMemcpyDeviceToHost, ctx->stream));
        YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const GbaRec &r = R->rec;
        const bool failed = r.status == YGZ_GBA_FAILED;
        long inl = 0;
        for (size_t c = 0; c < NC; ++c) inl += hpart[c];
        res->status[k] = r.status; res->lm_iterations[k] = r.lm_iterations; res->n_solves[k] = r.n_solves; res->cg_iterations[k] = r.cg_total;
        res->cg_capped[k] = r.cg_capped; res->inliers[k] = (int32_t)inl;
        res->cost_initial[k] = failed ? 0.0 : r.cost_initial; res->cost_final[k] = failed ? 0.0 : r.currentChi; res->lambda[k] = r.lambda;
        res->rounds_run = k + 1; res->launches = (int32_t)R->launches;
        if (failed) break;
    }
    uint8_t *h = (uint8_t *)hpart + ygz_round_up_256(NC * 4);
    const struct { size_t src, bytes; } parts[] = { { Y.t, N * 56 }, { Y.x, L * 24 }, { Y.outlier, E }, { Y.chi2, E * 8 } };
    for (const auto &q : parts) {
        YGZ_HIPCHK(ctx, hipMemcpyAsync(h, R->dev + q.src, q.bytes, hipMemcpyDeviceToHost, ctx->stream));
        h += ygz_round_up_256(q.bytes);
    }
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

}  // namespace

extern "C" {

void ygz_hip_default_sba_params(ygz_sba_params *p)
{
    if (!p) return;
    p->max_iterations = 10; p->max_trials = 10; p->cg_max_iterations = 0; p->cg_batch = 0;
    p->cg_tol = 1e-8; p->min_rel_decrease = 1e-9;
    p->baseline = 0.0; p->chi2_mono = 5.991; p->chi2_stereo = 7.815;
    p->rounds = 2; p->robust_rounds = 1;
    p->iterations[0] = 5; p->iterations[1] = 10; p->iterations[2] = 0; p->iterations[3] = 0;
}

int ygz_hip_stereo_ba(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points, int n_edges,
                      const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const uint8_t *kind, const int32_t *level,
                      const double K4[4], const ygz_sba_params *params, double *poses_out, double *points_out, uint8_t *outlier, double *chi2,
                      ygz_sba_result *result)
{
    if (!poses_out || !points_out || !result) return YGZ_E_INVALID;
    Run R;
    const SbaArgs a = { n_poses, poses, fixed, n_points, points, n_edges, edge_pose, edge_point, obs, kind, level, K4 };
    ygz_sba_result res;
    const int rc = run(ctx, a, params, false, &R, &res);
    if (rc != YGZ_OK) return rc;
    *result = res;
    const size_t N = (size_t)n_poses, L = (size_t)n_points, E = (size_t)n_edges, NC = (E + GBA_CHUNK - 1) / GBA_CHUNK;
    const bool failed = res.status[0] == YGZ_GBA_FAILED;
    const uint8_t *h = R.host + ygz_round_up_256(sizeof(GbaRec)) + ygz_round_up_256(NC * 4);
    memcpy(poses_out, failed ? (const void *)poses : (const void *)h, N * 56);
    h += ygz_round_up_256(N * 56);
    memcpy(points_out, failed ? (const void *)points : (const void *)h, L * 24);
    h += ygz_round_up_256(L * 24);
    if (outlier) memcpy(outlier, h, E);
    h += ygz_round_up_256(E);
    if (chi2) memcpy(chi2, h, E * 8);
    return YGZ_OK;
}

int ygz_hip_sba_linearize(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points,
                          int n_edges, const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const uint8_t *kind,
                          const int32_t *level, const double K4[4], const ygz_sba_params *params, double *residuals, double *weights, double *Jp,
                          double *Jl, double *Hpp, double *bp, double *Hll, double *bl, double *cost)
{
    Run R;
    const SbaArgs a = { n_poses, poses, fixed, n_points, points, n_edges, edge_pose, edge_point, obs, kind, level, K4 };
    const int rc = run(ctx, a, params, true, &R, nullptr);
    if (rc != YGZ_OK) return rc;
    const size_t N = (size_t)n_poses, L = (size_t)n_points, E = (size_t)n_edges;
    const uint8_t *h = R.host + ygz_round_up_256(sizeof(GbaRec));
    if (residuals) to_rows((const double *)h, E, 3, residuals);
    h += ygz_round_up_256(E * 24);
    if (weights) memcpy(weights, h, E * 8);
    h += ygz_round_up_256(E * 8);
    if (Jp) to_rows((const double *)h, E, 18, Jp);
    h += ygz_round_up_256(E * 144);
    if (Jl) to_rows((const double *)h, E, 9, Jl);
    h += ygz_round_up_256(E * 72);
    if (Hpp) memcpy(Hpp, h, N * 168);
    h += ygz_round_up_256(N * 168);
    if (bp) memcpy(bp, h, N * 48);
    h += ygz_round_up_256(N * 48);
    if (Hll) to_rows((const double *)h, L, 6, Hll);
    h += ygz_round_up_256(L * 48);
    if (bl) to_rows((const double *)h, L, 3, bl);
    if (cost) *cost = R.rec.cost_initial;
    return R.rec.status == YGZ_GBA_FAILED ? YGZ_E_STATE : YGZ_OK;
}

}  // extern "C"
