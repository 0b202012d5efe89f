// Global bundle adjustment after a loop closing (ORB-SLAM2's Optimizer::GlobalBundleAdjustemnt; nothing in the reference, whose loop closing is
// empty): all keyframe poses and map points against all observations, Levenberg-Marquardt with g2o's rules, every step solved on the
// point-marginalised (Schur) camera system by preconditioned conjugate gradients without ever forming that system.  The arithmetic is
// tests/gba_ref.c's decision by decision (-ffp-contract=off, only + - * / and sqrt), so every output is bit-identical to it (DESIGN.md
// section 15).  Unlike the pose graph (pgo.hip: one resident workgroup) the work is spread over many workgroups, one short kernel per phase on
// the context's stream; no kernel waits for another workgroup, and the control state of the LM and CG loops lives in a device record (GbaRec)
// that a kernel queued behind a finished solve or a decided trial reads before it returns at once.  The host queues CG iterations in batches
// and reads that record back once per batch.
//   k_gba_linearize      lane = edge (GBA_CHUNK per workgroup): residual, weight, Jacobian blocks, Hpl in both CSR orders, cost chunk sums
//   k_gba_point_system   lane = point: Hll, bl over the point's edges
//   k_gba_pose_system    workgroup = pose: Hpp, bp lane-strided over the pose's edges, then the tree
//   k_gba_begin          one workgroup: the cost, lambda_0, the record
//   k_gba_point_trial    lane = point: (Hll + lambda I)^-1 and its product with bl
//   k_gba_pose_trial     workgroup = pose: the reduced right-hand side and the factor of the pose's Schur diagonal block
//   k_gba_cg_begin       one workgroup: x = 0, r, z, p, r.z, the stop value
//   k_gba_cg_point       lane = point: v_l = Hinv sum Hpl^T p            (first half of S p)
//   k_gba_cg_pose        workgroup = pose: q = (Hpp + lambda I) p - sum Hpl v_l, and p.q per pose
//   k_gba_cg_step        one workgroup: alpha, x, r, z, beta, p, the record
//   k_gba_point_update   lane = point: the back-substitution, the trial points, the points' part of rho's denominator
//   k_gba_pose_update    lane = pose: the retraction, the poses' part of rho's denominator
//   k_gba_cost           lane = edge: the robust cost of the trial state
//   k_gba_decide         one workgroup: rho, accept or reject, lambda, the counters and the status
//   k_gba_accept         the trial state becomes the estimate
#define GBA_LANES 256                      // GB_LANES of tests/gba_ref.c: the lanes of the fixed summation order
#define GBA_CHUNK 1024                     // GB_CHUNK: elements per first-level chunk of a two-level sum
#define GBA_CG_CAP 1024                    // GB_CG_CAP: bound of the automatic CG cap
#include "gba_phases.h"                    // the eleven phases that do not see the edge model, and the host driver (shared with sba.hip)

namespace {

// ---- the four phases that see the edge model -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBA_LANES) void k_gba_linearize(GbaDev D, int gated)
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
        const int v = D.edge_pose[e], l = D.edge_point[e];
        double T[7], X[3], ob[2], r[2], w, rho, Jp[12], Jl[6];
#pragma unroll
        for (int k = 0; k < 7; ++k) T[k] = D.T[7 * v + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = D.X[3 * (size_t)l + k];
        ob[0] = D.obs[2 * (size_t)e]; ob[1] = D.obs[2 * (size_t)e + 1];
        bad |= !gb_edge_terms(T, X, ob, K, in.delta, r, &w, &rho, Jp, Jl);
        acc += rho;
        D.res[e] = r[0]; D.res[E + e] = r[1];
        D.w[e] = w;
#pragma unroll
        for (int k = 0; k < 12; ++k) D.Jp[k * E + e] = Jp[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) D.Jl[k * E + e] = Jl[k];
        const size_t sp = (size_t)D.slot_p[e], sl = (size_t)D.slot_l[e];
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const double h = w * (Jp[a] * Jl[b] + Jp[6 + a] * Jl[3 + b]);
                D.HplP[(3 * a + b) * E + sp] = h;
                D.HplL[(3 * a + b) * E + sl] = h;
            }
    }
    gba_reduce<1>(sh, &acc);
    if (threadIdx.x == 0) D.cpart[blockIdx.x] = sh.out[0];
    if (bad) atomicOr(&D.rec->bad_lin, 1);
}

__global__ __launch_bounds__(GBA_LANES) void k_gba_point_system(GbaDev D, int gated)
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
        double J[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) J[k] = D.Jl[k * E + e];
        const double r0 = D.res[e], r1 = D.res[E + e], w = D.w[e];
        int m = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = a; b < 3; ++b) h[m++] += w * (J[a] * J[b] + J[3 + a] * J[3 + b]);
            g[a] += w * (J[a] * r0 + J[3 + a] * r1);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) D.Hll[k * L + l] = h[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) D.bl[k * L + l] = -g[k];
    gba_max_diag(D.rec, h[0]); gba_max_diag(D.rec, h[3]); gba_max_diag(D.rec, h[5]);
}

__global__ __launch_bounds__(GBA_LANES) void k_gba_pose_system(GbaDev D, int gated)
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
        double J[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) J[k] = D.Jp[k * E + e];
        const double r0 = D.res[e], r1 = D.res[E + e], w = D.w[e];
        int m = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
#pragma unroll
            for (int b = a; b < 6; ++b) acc[m++] += w * (J[a] * J[b] + J[6 + a] * J[6 + b]);
            acc[21 + a] += w * (J[a] * r0 + J[6 + a] * r1);
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

__global__ __launch_bounds__(GBA_LANES) void k_gba_cost(GbaDev D)
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
        const int v = D.edge_pose[e], l = D.edge_point[e];
        double T[7], X[3], ob[2], R[9], P[3], r[2], w, term = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) T[k] = D.Tn[7 * v + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) X[k] = D.Xn[3 * (size_t)l + k];
        ob[0] = D.obs[2 * (size_t)e]; ob[1] = D.obs[2 * (size_t)e + 1];
        if (!gb_residual(T, X, ob, K, R, P, r)) bad = 1;
        else gb_robust(r, in.delta, &term, &w);
        acc += term;
    }
    gba_reduce<1>(sh, &acc);
    if (threadIdx.x == 0) D.cpart[blockIdx.x] = sh.out[0];
    if (bad) atomicOr(&D.rec->bad_cost, 1);
}

// ---- the other eleven: gba_phases.h ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GBA_LANES) void k_gba_begin(GbaDev D) { gba_ph_begin(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_point_trial(GbaDev D) { gba_ph_point_trial(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_pose_trial(GbaDev D) { gba_ph_pose_trial(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_cg_begin(GbaDev D) { gba_ph_cg_begin(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_cg_point(GbaDev D) { gba_ph_cg_point(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_cg_pose(GbaDev D) { gba_ph_cg_pose(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_cg_step(GbaDev D) { gba_ph_cg_step(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_point_update(GbaDev D) { gba_ph_point_update(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_pose_update(GbaDev D) { gba_ph_pose_update(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_decide(GbaDev D) { gba_ph_decide(D); }
__global__ __launch_bounds__(GBA_LANES) void k_gba_accept(GbaDev D) { gba_ph_accept(D); }

const GbaKernels KERNELS = { k_gba_linearize, k_gba_point_system, k_gba_pose_system, k_gba_begin, k_gba_point_trial, k_gba_pose_trial, k_gba_cg_begin,
                             k_gba_cg_point, k_gba_cg_pose, k_gba_cg_step, k_gba_point_update, k_gba_pose_update, k_gba_cost, k_gba_decide,
                             k_gba_accept };

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// every refusal of the header, in its order, before anything touches the device
int validate(const ygz_hip_ctx *ctx, int n, const double *poses, const uint8_t *fixed, int nl, const double *points, int ne,
             const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const double *K4, double huber_delta, const ygz_gba_params &p)
{
    if (!poses || !fixed || !points || !edge_pose || !edge_point || !obs || !K4) return YGZ_E_INVALID;
    if (n > YGZ_GBA_MAX_POSES || nl > YGZ_GBA_MAX_POINTS || ne > YGZ_GBA_MAX_EDGES) return YGZ_E_CAPACITY;
    if (n < 2 || nl < 1 || ne < 1) return YGZ_E_INVALID;
    if (p.max_iterations < 1 || p.max_iterations > 1000 || p.max_trials < 1 || p.max_trials > 100 || p.cg_max_iterations < 0
        || p.cg_max_iterations > 65536 || p.cg_batch < 0 || p.cg_batch > 1024 || !(p.cg_tol > 0 && p.cg_tol < 1)
        || !(p.min_rel_decrease >= 0 && p.min_rel_decrease < 1))
        return YGZ_E_INVALID;
    if (!finite_n(K4, 4) || !(K4[0] > 0) || !(K4[1] > 0) || !(std::fabs(huber_delta) <= GB_DMAX)) return YGZ_E_INVALID;
    std::vector<int32_t> deg_pose(n, 0), deg_point(nl, 0);
    for (int e = 0; e < ne; ++e) {
        const int v = edge_pose[e], l = edge_point[e];
        if (v < 0 || v >= n || l < 0 || l >= nl) return YGZ_E_INVALID;
        ++deg_pose[v]; ++deg_point[l];
    }
    if (!finite_n(obs, 2 * (size_t)ne) || !finite_n(poses, 7 * (size_t)n) || !finite_n(points, 3 * (size_t)nl)) return YGZ_E_INVALID;
    int n_free = 0;
    for (int v = 0; v < n; ++v) {
        const double *q = poses + 7 * (size_t)v;
        if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0)) return YGZ_E_INVALID;
        if (fixed[v]) continue;
        ++n_free;
        if (!deg_pose[v]) return YGZ_E_INVALID;
    }
    if (n_free < 1) return YGZ_E_INVALID;
    for (int l = 0; l < nl; ++l) if (deg_point[l] < 2) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    return YGZ_OK;
}

// validation, then the shared driver: the CSR lists, one upload, the launches with one small read-back per batch of CG iterations, the wait.
// stage: the linearisation alone.  Afterwards the page-locked area holds the results
int run(ygz_hip_ctx *ctx, int n, const double *poses, const uint8_t *fixed, int nl, const double *points, int ne, const int32_t *edge_pose,
        const int32_t *edge_point, const double *obs, const double *K4, double huber_delta, const ygz_gba_params *params, bool stage, Run *R)
{
    ygz_gba_params p;
    if (params) p = *params; else ygz_hip_default_gba_params(&p);
    const int rv = validate(ctx, n, poses, fixed, nl, points, ne, edge_pose, edge_point, obs, K4, huber_delta, p);
    if (rv != YGZ_OK) return rv;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    const size_t N = (size_t)n, L = (size_t)nl, E = (size_t)ne;
    // one page-locked block: the upload's image, and behind it the area the results come back into
    YgzBlobLayout down;
    down.add(sizeof(GbaRec));
    if (stage) for (size_t bytes : { E * 16, E * 8, E * 96, E * 48, N * 168, N * 48, L * 48, L * 24 }) down.add(bytes);
    else { down.add(N * 56); down.add(L * 24); }
    GbaIn in;
    memset(&in, 0, sizeof in);
    in.delta = huber_delta; in.cg_tol = p.cg_tol; in.min_rel_decrease = p.min_rel_decrease;
    in.max_iterations = p.max_iterations; in.max_trials = p.max_trials; in.stage_only = stage ? 1 : 0;
    const GbaProblem pb = { n, nl, ne, 2, poses, points, obs, K4, fixed, edge_pose, edge_point, nullptr, nullptr };
    int rc = gba_open(ctx, SCR_GBA, pb, in, p.cg_max_iterations, down.end, R);
    if (rc != YGZ_OK) return rc;
    if ((rc = gba_linearize_first(ctx, KERNELS, R)) != YGZ_OK) return rc;
    if (stage) return gba_fetch_stage(ctx, R, 2);
    if ((rc = gba_solve(ctx, KERNELS, R, p.max_iterations, p.max_trials, p.cg_batch)) != YGZ_OK) return rc;
    uint8_t *h = R->host + ygz_round_up_256(sizeof(GbaRec));
    YGZ_HIPCHK(ctx, hipMemcpyAsync(h, R->dev + R->Y.t, N * 56, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipMemcpyAsync(h + ygz_round_up_256(N * 56), R->dev + R->Y.x, L * 24, hipMemcpyDeviceToHost, ctx->stream));
    YGZ_HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return YGZ_OK;
}

}  // namespace

extern "C" {

void ygz_hip_default_gba_params(ygz_gba_params *p)
{
    if (!p) return;
    p->max_iterations = 10; p->max_trials = 10; p->cg_max_iterations = 0; p->cg_batch = 0;
    p->cg_tol = 1e-8; p->min_rel_decrease = 1e-9;
}

int ygz_hip_global_ba(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points, int n_edges,
                      const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const double K4[4], double huber_delta,
                      const ygz_gba_params *params, double *poses_out, double *points_out, ygz_gba_result *result)
{
    if (!poses_out || !points_out || !result) return YGZ_E_INVALID;
    Run R;
    const int rc = run(ctx, n_poses, poses, fixed, n_points, points, n_edges, edge_pose, edge_point, obs, K4, huber_delta, params, false, &R);
    if (rc != YGZ_OK) return rc;
    const GbaRec &r = R.rec;
    const bool failed = r.status == YGZ_GBA_FAILED;
    result->cost_initial = failed ? 0.0 : r.cost_initial; result->cost_final = failed ? 0.0 : r.currentChi; result->lambda = r.lambda;
    result->status = r.status; result->lm_iterations = r.lm_iterations; result->n_solves = r.n_solves;
    result->cg_iterations_total = r.cg_total; result->cg_capped = r.cg_capped; result->pad = 0;
    const size_t N = (size_t)n_poses, L = (size_t)n_points;
    const uint8_t *h = R.host + ygz_round_up_256(sizeof(GbaRec));
    memcpy(poses_out, failed ? (const void *)poses : (const void *)h, N * 56);
    memcpy(points_out, failed ? (const void *)points : (const void *)(h + ygz_round_up_256(N * 56)), L * 24);
    return YGZ_OK;
}

int ygz_hip_gba_linearize(ygz_hip_ctx *ctx, int n_poses, const double *poses, const uint8_t *fixed, int n_points, const double *points,
                          int n_edges, const int32_t *edge_pose, const int32_t *edge_point, const double *obs, const double K4[4],
                          double huber_delta, const ygz_gba_params *params, double *residuals, double *weights, double *Jp, double *Jl,
                          double *Hpp, double *bp, double *Hll, double *bl, double *cost)
{
    Run R;
    const int rc = run(ctx, n_poses, poses, fixed, n_points, points, n_edges, edge_pose, edge_point, obs, K4, huber_delta, params, true, &R);
    if (rc != YGZ_OK) return rc;
    const size_t N = (size_t)n_poses, L = (size_t)n_points, E = (size_t)n_edges;
    const uint8_t *h = R.host + ygz_round_up_256(sizeof(GbaRec));
    if (residuals) to_rows((const double *)h, E, 2, residuals);
    h += ygz_round_up_256(E * 16);
    if (weights) memcpy(weights, h, E * 8);
    h += ygz_round_up_256(E * 8);
    if (Jp) to_rows((const double *)h, E, 12, Jp);
    h += ygz_round_up_256(E * 96);
    if (Jl) to_rows((const double *)h, E, 6, Jl);
    h += ygz_round_up_256(E * 48);
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
