// P0 -- stereo pose optimisation: ORB-SLAM2's Optimizer::PoseOptimization for a batch of frames.  Mono edges (u, v) and stereo edges (u, v, uR)
// against one free pose, g2o's Huber kernel on chi2, the information scaled by the pyramid level (w = 4^-level), rounds of Levenberg-Marquardt
// with g2o's rules from the entry pose, and a re-classification of every edge after each round.  The frozen spec is tests/popt_ref.c
// (DESIGN.md section 20): uncontracted + - * / and sqrt in FP64, every sum in one stated order, and every output is bit-identical to it.
//   k_pose_opt   one workgroup of 256 lanes per frame, all frames of the call in one launch; all rounds, iterations, trials and classifications
//                inside the launch.  The lanes stride over the frame's edges (lane l: edges l, l + 256, ... in that order); a pass ends in a
//                fixed-order reduction (21 + 6 + 1 sums for a linearisation, 1 for a cost-only trial: the rows of 16 lanes by DPP, the rows and
//                then the four wavefronts in order); lane 0 does the 6 x 6 Cholesky and the LM bookkeeping in LDS; what every lane branches on
//                is read between two barriers.
// Integer LDS counters only (accepted / rejected edges of a pass, inliers): no output depends on scheduling.  No floating-point atomic, no wait
// for another workgroup, no scratch, no environment switch.  The edges are fetched per pass (no register cache): a frame of any length takes the
// same path.
#include "ygz_internal.h"
#include "popt_dev.h"                   // PoptArgs and the kernel's prototype: svo.hip launches it too
#include "posemath_dev.h"               // rotation, retraction T <- Delta(d) o T (pr_retract), level weight
#include <math.h>
#include <string.h>
#pragma clang fp contract(off)

#define PT_THREADS 256
#define PT_NV 28
#define PT_DMAX 1.7976931348623157e308

static_assert(PT_THREADS == PT_DEV_THREADS, "popt_dev.h states this file's block size");

enum { PT_PH_LIN = 0, PT_PH_TRIAL = 1, PT_PH_DONE = 2 };

// the shared state of a frame's solve: written by lane 0 between barriers
struct PoptState {
    double entry[7], T[7], Tn[7];
    double H[21], b[6];
    double lambda, ni, chi, scale, rho;
    int it, iters, qmax, converged, status, phase, nrej_lin;
    int c_ok, c_rej, c_inl;             // the integer counters of a pass and of a classification
    double K[5], d2m, d2s, dm, ds, min_rel_decrease;    // the call's constants, out of the scalar registers
};

// P = R X + t and the residuals (pr_residual); false when the edge is rejected
__device__ __forceinline__ bool pt_residual(const double *R, const double *t, const double *X, const double *ob, int kind, const double *K, double *P,
                                            double *r)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) P[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2]) + t[i];
    if (!(P[2] > 0)) return false;
    const double xn = P[0] / P[2], yn = P[1] / P[2], up = K[0] * xn + K[2];
    r[0] = ob[0] - up;
    r[1] = ob[1] - (K[1] * yn + K[3]);
    r[2] = 0.0;
    if (kind == 2) r[2] = ob[2] - (up - K[4] / P[2]);
    return fabs(r[0]) <= PT_DMAX && fabs(r[1]) <= PT_DMAX && fabs(r[2]) <= PT_DMAX;
}

__device__ __forceinline__ double pt_chi2(const double *r, int kind, double w)
{
    double e2 = r[0] * r[0] + r[1] * r[1];
    if (kind == 2) e2 = e2 + r[2] * r[2];
    return w * e2;
}

// g2o's RobustKernelHuber on chi2 (pr_robust)
__device__ __forceinline__ void pt_robust(double chi2, double d2, double delta, double *rho0, double *rho1)
{
    *rho0 = chi2; *rho1 = 1.0;
    if (d2 > 0 && chi2 > d2) {
        const double s = sqrt(chi2);
        *rho0 = 2.0 * s * delta - d2;
        *rho1 = delta / s;
    }
}

// one edge's share of a pass (pr_edge_terms / pr_edge_cost); false when it is rejected (nothing is added)
__device__ __forceinline__ bool pt_edge(const double *R, const double *t, const double *X, const double *ob, int level, int kind, const double *K,
                                        double d2, double delta, bool full, double *acc)
{
    double P[3], r[3], rho0, rho1;
    if (!pt_residual(R, t, X, ob, kind, K, P, r)) return false;
    const double w = ygz_level_weight(level);
    pt_robust(pt_chi2(r, kind, w), d2, delta, &rho0, &rho1);
    if (full) {
        double J[18];
        const double x = P[0], y = P[1], z = P[2];
        const double iz = 1.0 / z, a = K[0] * iz, b = K[1] * iz, c = K[0] * (x / z) * iz, d = K[1] * (y / z) * iz;
        J[0] = c * y;         J[1] = -(a * z) - c * x; J[2] = a * y;    J[3] = -a;  J[4] = 0.0; J[5] = c;
        J[6] = b * z + d * y; J[7] = -(d * x);         J[8] = -(b * x); J[9] = 0.0; J[10] = -b; J[11] = d;
#pragma unroll
        for (int k = 0; k < 6; ++k) J[12 + k] = 0.0;
        if (kind == 2) {
            const double e = (K[4] * iz) * iz;
            J[12] = J[0] - e * y; J[13] = J[1] + e * x; J[14] = J[2]; J[15] = J[3]; J[16] = 0.0; J[17] = J[5] - e;
        }
        const double ww = rho1 * w;
        int m = 0;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
#pragma unroll
            for (int v = u; v < 6; ++v) {
                double h = J[u] * J[v] + J[6 + u] * J[6 + v];
                if (kind == 2) h = h + J[12 + u] * J[12 + v];
                acc[m] += ww * h;
                ++m;
            }
            double g = J[u] * r[0] + J[6 + u] * r[1];
            if (kind == 2) g = g + J[12 + u] * r[2];
            acc[21 + u] += ww * g;
        }
    }
    acc[27] += rho0;
    return true;
}

// One pass over the frame's active edges at `pose` (LDS): sum [0..20] the upper triangle of sum rho' w J^T J, sum [21..26] sum rho' w J^T r,
// sum [27] the cost (full == false: the cost alone); S.c_ok / S.c_rej count the accepted and the rejected active edges (lane 0 zeroes them after
// it has read them).  Fixed order: the lanes' partial sums, per wavefront the rows of 16 by the tree over adjacent lanes, ((r0 + r1) + r2) + r3,
// then the four wavefronts in order (pr_reduce).  Ends behind a barrier.
__device__ __forceinline__ void pt_pass(const PoptArgs &A, PoptState &S, int beg, int n, const double *pose, bool full, bool robust, double (*red)[PT_NV],
                                        double *sum)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double R[9], t[3], K[5];
    ygz_quat_rotation(pose, R);
    t[0] = pose[4]; t[1] = pose[5]; t[2] = pose[6];
#pragma unroll
    for (int k = 0; k < 5; ++k) K[k] = S.K[k];
    const double d2m = robust ? S.d2m : 0.0, d2s = robust ? S.d2s : 0.0, dm = S.dm, ds = S.ds;
    double acc[PT_NV];
#pragma unroll
    for (int i = 0; i < PT_NV; ++i) acc[i] = 0.0;
    int n_ok = 0, n_rej = 0;
    for (int i = tid; i < n; i += PT_THREADS) {
        const size_t g = (size_t)(beg + i);
        const int kind = A.kind[g];
        if (kind == 0 || A.outlier[g]) continue;
        const double X[3] = { A.pw[3 * g], A.pw[3 * g + 1], A.pw[3 * g + 2] }, ob[3] = { A.obs[3 * g], A.obs[3 * g + 1], A.obs[3 * g + 2] };
        if (pt_edge(R, t, X, ob, A.level[g], kind, K, kind == 2 ? d2s : d2m, kind == 2 ? ds : dm, full, acc)) ++n_ok; else ++n_rej;
    }
    if (full) {
        ygz_wave_sums_d(acc);                                    // the totals are in lanes 48 .. 63
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < PT_NV; ++i) red[wv][i] = acc[i];
        }
    } else {
        const double v = ygz_wave_sum_d(acc[27]);
        if (lane == 0) red[wv][27] = v;
    }
    if (n_ok) atomicAdd(&S.c_ok, n_ok);
    if (n_rej) atomicAdd(&S.c_rej, n_rej);
    __syncthreads();
    if (tid >= (full ? 0 : 27) && tid < PT_NV) sum[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
}

// x = (H + lambda I)^-1 b by a dense Cholesky (pr_solve6); false on a non-positive or non-finite pivot
__device__ bool pt_solve6(const double *H, double lambda, const double *b, double *x)
{
    double Am[36], L[36], y[6];
    int m = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) { Am[a * 6 + c] = H[m]; Am[c * 6 + a] = H[m]; ++m; }
    for (int a = 0; a < 6; ++a) Am[a * 7] = Am[a * 7] + lambda;
    for (int k = 0; k < 36; ++k) L[k] = 0.0;
    for (int j = 0; j < 6; ++j) {
        double d = Am[j * 6 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0 && d <= PT_DMAX)) return false;
        const double ljj = sqrt(d);
        L[j * 6 + j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double v = Am[i * 6 + j];
            for (int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = v / ljj;
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= L[i * 6 + k] * y[k];
        y[i] = v / L[i * 6 + i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k * 6 + i] * x[k];
        x[i] = v / L[i * 6 + i];
    }
    return true;
}

// The end of one trial (lane 0): the gain ratio and g2o's update of lambda.  `ok` is false for a failed trial (tempChi = DMAX, scale = 0 then).
// Returns whether the trial loop of this iteration goes on.
__device__ bool pt_finish_trial(const PoptArgs &A, PoptState &S, bool ok, double tempChi, double scale)
{
    scale += 1e-3;
    double rho = (S.chi - tempChi) / scale;
    if (!(fabs(rho) <= PT_DMAX)) rho = -1.0;
    S.rho = rho;
    if (ok && rho > 0) {
        const double u = 2.0 * rho - 1.0;
        double alpha = 1.0 - u * u * u;
        if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
        S.lambda = S.lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
        S.ni = 2.0;
        S.converged = S.chi - tempChi <= S.min_rel_decrease * S.chi;
        S.chi = tempChi;
        for (int k = 0; k < 7; ++k) S.T[k] = S.Tn[k];
    } else {
        S.lambda = S.lambda * S.ni; S.ni = S.ni * 2.0;
        if (!(fabs(S.lambda) <= PT_DMAX)) return false;
    }
    ++S.qmax;
    return rho < 0 && S.qmax < A.max_trials;
}

// The end of an iteration (lane 0): the next phase
__device__ void pt_end_iteration(const PoptArgs &A, PoptState &S)
{
    ++S.iters;
    if (S.qmax == A.max_trials || S.rho == 0 || !(fabs(S.lambda) <= PT_DMAX)) { S.status = YGZ_POPT_STALLED; S.phase = PT_PH_DONE; return; }
    if (S.converged) { S.status = YGZ_POPT_CONVERGED; S.phase = PT_PH_DONE; return; }
    ++S.it;
    S.phase = S.it < A.iters ? PT_PH_LIN : PT_PH_DONE;         // the iterations ran out: the status stays MAX_ITERATIONS
}

// Trials until one needs a cost pass (S.Tn and S.scale are ready, phase TRIAL) or the iteration ends (lane 0)
__device__ void pt_next_trial(const PoptArgs &A, PoptState &S)
{
    for (;;) {
        double d[6];
        if (pt_solve6(S.H, S.lambda, S.b, d)) {
            bool zero = true;
            double scale = 0.0;
            for (int a = 0; a < 6; ++a) { zero = zero && d[a] == 0.0; scale += d[a] * (S.lambda * d[a] + S.b[a]); }
            if (zero) { for (int k = 0; k < 7; ++k) S.Tn[k] = S.T[k]; }
            else ygz_se3_retract(S.T, d, S.Tn);
            S.scale = scale;
            S.phase = PT_PH_TRIAL;
            return;
        }
        if (!pt_finish_trial(A, S, false, PT_DMAX, 0.0)) { pt_end_iteration(A, S); return; }
    }
}

__global__ __launch_bounds__(PT_THREADS) void k_pose_opt(PoptArgs A)
{
    __shared__ double red[4][PT_NV];
    __shared__ double sum[PT_NV];
    __shared__ PoptState S;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int beg = A.off[f], n = (A.end ? A.end[f] : A.off[f + 1]) - beg;
    const size_t fr = (size_t)f * YGZ_POPT_MAX_ROUNDS;
    if (tid < 7) { const double v = A.poses[7 * (size_t)f + tid]; S.entry[tid] = v; S.T[tid] = v; }
    if (tid == 0) {
        S.c_ok = 0; S.c_rej = 0; S.c_inl = 0;
        for (int q = 0; q < 5; ++q) S.K[q] = A.K[q];
        S.d2m = A.d2m; S.d2s = A.d2s; S.dm = A.dm; S.ds = A.ds; S.min_rel_decrease = A.min_rel_decrease;
    }
    for (int i = tid; i < n; i += PT_THREADS) A.outlier[beg + i] = 0;      // round 0: every edge with kind != 0 is active
    __syncthreads();

    int run = 0, inl = 0;
    for (int k = 0; k < A.rounds; ++k) {
        const bool robust = k < A.robust_rounds;
        if (tid < 7) S.T[tid] = S.entry[tid];
        if (tid == 0) {
            S.lambda = 0.0; S.ni = 2.0; S.chi = 0.0; S.it = 0; S.iters = 0; S.status = YGZ_POPT_MAX_ITERATIONS; S.phase = PT_PH_LIN;
            A.cost_initial[fr + k] = 0.0;
        }
        __syncthreads();
        for (;;) {
            const int ph = S.phase;                              // block-uniform: read between two barriers
            if (ph == PT_PH_DONE) break;
            const bool full = ph == PT_PH_LIN;
            pt_pass(A, S, beg, n, full ? S.T : S.Tn, full, robust, red, sum);
            if (tid == 0) {
                const int n_ok = S.c_ok, n_rej = S.c_rej;
                S.c_ok = 0; S.c_rej = 0;
                if (full) {                                      // the linearisation of iteration S.it
                    S.nrej_lin = n_rej;
                    if (S.it == 0 && (n_ok < A.min_edges || !(fabs(sum[27]) <= PT_DMAX))) { S.status = YGZ_POPT_FAILED; S.phase = PT_PH_DONE; }
                    else {
                        if (S.it == 0) A.cost_initial[fr + k] = sum[27];
                        S.chi = sum[27];
                        for (int a = 0; a < 21; ++a) S.H[a] = sum[a];
                        for (int a = 0; a < 6; ++a) S.b[a] = -sum[21 + a];
                        if (S.it == 0) {
                            double mx = 0.0;
                            int m = 0;
                            for (int a = 0; a < 6; ++a) { const double h = fabs(sum[m]); if (h > mx) mx = h; m += 6 - a; }
                            S.lambda = 1e-5 * mx; S.ni = 2.0;
                        }
                        S.rho = 0.0; S.qmax = 0; S.converged = 0;
                        pt_next_trial(A, S);
                    }
                } else {                                         // the cost of the trial pose
                    double tempChi = sum[27], scale = S.scale;
                    const bool ok = n_rej <= S.nrej_lin && fabs(tempChi) <= PT_DMAX;
                    if (!ok) { tempChi = PT_DMAX; scale = 0.0; }
                    if (pt_finish_trial(A, S, ok, tempChi, scale)) pt_next_trial(A, S);
                    else pt_end_iteration(A, S);
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            A.status[fr + k] = S.status; A.iterations[fr + k] = S.iters; A.lambda[fr + k] = S.lambda;
            A.cost_final[fr + k] = S.status == YGZ_POPT_FAILED ? 0.0 : S.chi;
        }
        // ---------------- the classification of every edge with kind != 0 at the round's pose, by a fresh evaluation
        {
            double R[9], t[3], K[5];
            ygz_quat_rotation(S.T, R);
            t[0] = S.T[4]; t[1] = S.T[5]; t[2] = S.T[6];
#pragma unroll
            for (int q = 0; q < 5; ++q) K[q] = S.K[q];
            int mine = 0;
            for (int i = tid; i < n; i += PT_THREADS) {
                const size_t g = (size_t)(beg + i);
                const int kind = A.kind[g];
                if (kind == 0) { A.chi2[g] = -1.0; A.outlier[g] = 0; continue; }
                const double X[3] = { A.pw[3 * g], A.pw[3 * g + 1], A.pw[3 * g + 2] }, ob[3] = { A.obs[3 * g], A.obs[3 * g + 1], A.obs[3 * g + 2] };
                double P[3], r[3];
                if (!pt_residual(R, t, X, ob, kind, K, P, r)) { A.chi2[g] = 0.0; A.outlier[g] = 1; continue; }
                const double c = pt_chi2(r, kind, ygz_level_weight(A.level[g]));
                const bool out = c > (kind == 2 ? S.d2s : S.d2m);
                A.chi2[g] = c; A.outlier[g] = (uint8_t)out;
                if (!out) ++mine;
            }
            if (mine) atomicAdd(&S.c_inl, mine);
        }
        __syncthreads();
        inl = S.c_inl;
        run = k + 1;
        __syncthreads();                                         // every lane has read the count before lane 0 clears it
        if (tid == 0) S.c_inl = 0;
        if (inl < A.min_inliers) break;
    }
    if (tid < 7) A.poses[7 * (size_t)f + tid] = S.T[tid];
    if (tid == 0) {
        A.inliers[f] = inl; A.rounds_run[f] = run;
        for (int k = run; k < YGZ_POPT_MAX_ROUNDS; ++k) {         // unused rounds are zero
            A.status[fr + k] = 0; A.iterations[fr + k] = 0; A.cost_initial[fr + k] = 0.0; A.cost_final[fr + k] = 0.0; A.lambda[fr + k] = 0.0;
        }
    }
}

void ygz_hip_default_pose_opt_params(ygz_pose_opt_params *p)
{
    if (!p) return;
    p->baseline = 0.0; p->chi2_mono = 5.991; p->chi2_stereo = 7.815;
    p->rounds = 4; p->iterations = 10; p->max_trials = 10; p->robust_rounds = 3; p->min_edges = 3; p->min_inliers = 10;
    p->min_rel_decrease = 0.0;
}

static size_t pt_up8(size_t v) { return (v + 7) & ~(size_t)7; }

extern "C" int ygz_hip_optimize_pose_stereo(ygz_hip_ctx *ctx, int n_frames, const int32_t *frame_off, const double *pw, const double *obs,
                                            const int32_t *level, const uint8_t *kind, const ygz_pose_opt_params *params, double *poses_io,
                                            uint8_t *outlier, double *chi2, int32_t *inliers, int32_t *rounds_run, int32_t *round_status,
                                            int32_t *round_iterations, double *round_cost_initial, double *round_cost_final, double *round_lambda)
{
    // every check before the device is touched; the context last, so that a null context refuses a valid call too
    if (!params || n_frames < 0 || !frame_off) return YGZ_E_INVALID;
    const ygz_pose_opt_params &p = *params;
    if (!isfinite(p.baseline) || !ygz_pose_params_ok(p)) return YGZ_E_INVALID;
    if (frame_off[0] != 0) return YGZ_E_INVALID;
    for (int f = 0; f < n_frames; ++f) if (frame_off[f + 1] < frame_off[f]) return YGZ_E_INVALID;
    const size_t n = (size_t)frame_off[n_frames], nz = n > 0 ? n : 1;
    if (n_frames > 0 && !poses_io) return YGZ_E_INVALID;
    if (n > 0 && (!pw || !obs || !level || !kind)) return YGZ_E_INVALID;
    bool stereo = false;
    for (size_t i = 0; i < n; ++i) {
        if (kind[i] > 2) return YGZ_E_INVALID;
        stereo = stereo || kind[i] == 2;
    }
    if (stereo && !(p.baseline > 0.0)) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    for (size_t i = 0; i < n; ++i) if (level[i] < 0 || level[i] >= ctx->prm.pyramid_levels) return YGZ_E_INVALID;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    if (n_frames == 0) return YGZ_OK;

    const size_t F = (size_t)n_frames, R8 = F * YGZ_POPT_MAX_ROUNDS;
    const size_t b_off = pt_up8((F + 1) * 4), b_pw = nz * 24, b_obs = nz * 24, b_level = pt_up8(nz * 4), b_kind = pt_up8(nz);
    const size_t b_pose = F * 56, b_chi2 = nz * 8, b_rd = R8 * 8, b_ri = pt_up8(R8 * 4), b_cnt = pt_up8(F * 4), b_out = pt_up8(nz);
    const size_t total = b_off + b_pw + b_obs + b_level + b_kind + b_pose + b_chi2 + 3 * b_rd + 2 * b_ri + 2 * b_cnt + b_out;
    void *blob = nullptr;
    int rc = ygz_scratch(ctx, SCR_GEN_0, total + 64, &blob);
    if (rc != YGZ_OK) return rc;
    uint8_t *hb = nullptr;
    if ((rc = ygz_scratch_mirror(ctx, SCR_GEN_0, (void **)&hb)) != YGZ_OK) return rc;
    // the inputs, then the outputs (the tail of the blob): one packed upload, one copy back
    size_t o = 0;
    const size_t o_off = o; o += b_off;
    const size_t o_pw = o; o += b_pw;
    const size_t o_obs = o; o += b_obs;
    const size_t o_level = o; o += b_level;
    const size_t o_kind = o; o += b_kind;
    const size_t o_pose = o; o += b_pose;
    const size_t o_chi2 = o; o += b_chi2;
    const size_t o_ci = o; o += b_rd;
    const size_t o_cf = o; o += b_rd;
    const size_t o_lam = o; o += b_rd;
    const size_t o_st = o; o += b_ri;
    const size_t o_it = o; o += b_ri;
    const size_t o_inl = o; o += b_cnt;
    const size_t o_run = o; o += b_cnt;
    const size_t o_out = o; o += b_out;
    uint8_t *db = (uint8_t *)blob;
    memcpy(hb + o_off, frame_off, (F + 1) * 4);
    if (n > 0) { memcpy(hb + o_pw, pw, n * 24); memcpy(hb + o_obs, obs, n * 24); memcpy(hb + o_level, level, n * 4); memcpy(hb + o_kind, kind, n); }
    memcpy(hb + o_pose, poses_io, b_pose);
    if ((rc = ygz_kcopy(ctx, db, hb, o_pose + b_pose, hipMemcpyHostToDevice)) != YGZ_OK) return rc;

    PoptArgs A;
    A.off = (const int32_t *)(db + o_off); A.end = nullptr; A.pw = (const double *)(db + o_pw); A.obs = (const double *)(db + o_obs);
    A.level = (const int32_t *)(db + o_level); A.kind = db + o_kind;
    A.poses = (double *)(db + o_pose); A.chi2 = (double *)(db + o_chi2);
    A.cost_initial = (double *)(db + o_ci); A.cost_final = (double *)(db + o_cf); A.lambda = (double *)(db + o_lam);
    A.status = (int32_t *)(db + o_st); A.iterations = (int32_t *)(db + o_it);
    A.inliers = (int32_t *)(db + o_inl); A.rounds_run = (int32_t *)(db + o_run);
    A.outlier = db + o_out;
    const double K4[4] = { (double)ctx->prm.fx, (double)ctx->prm.fy, (double)ctx->prm.cx, (double)ctx->prm.cy };
    ygz_popt_set_params(A, K4, p.baseline, p);
    YGZ_LAUNCH(ctx, KID_POSE_OPT, k_pose_opt, dim3((unsigned)n_frames), dim3(PT_THREADS), A);
    YGZ_HIPCHK(ctx, hipGetLastError());
    if ((rc = ygz_kcopy(ctx, hb + o_pose, db + o_pose, o - o_pose, hipMemcpyDeviceToHost)) != YGZ_OK) return rc;
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(poses_io, hb + o_pose, b_pose);
    if (n > 0 && outlier) memcpy(outlier, hb + o_out, n);
    if (n > 0 && chi2) memcpy(chi2, hb + o_chi2, n * 8);
    if (inliers) memcpy(inliers, hb + o_inl, F * 4);
    if (rounds_run) memcpy(rounds_run, hb + o_run, F * 4);
    if (round_status) memcpy(round_status, hb + o_st, R8 * 4);
    if (round_iterations) memcpy(round_iterations, hb + o_it, R8 * 4);
    if (round_cost_initial) memcpy(round_cost_initial, hb + o_ci, R8 * 8);
    if (round_cost_final) memcpy(round_cost_final, hb + o_cf, R8 * 8);
    if (round_lambda) memcpy(round_lambda, hb + o_lam, R8 * 8);
    return YGZ_OK;
}
