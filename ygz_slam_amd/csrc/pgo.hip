// Loop correction's optimiser -- Sim3 pose-graph optimisation (ORB-SLAM2's Optimizer::OptimizeEssentialGraph; nothing in the reference, whose
// loop closing is empty).  The arithmetic is tests/pgo_ref.c's decision by decision (-ffp-contract=off, only + - * / and sqrt), so every
// output is bit-identical to it.  One call = one upload, one launch on the context's stream, one copy back, one wait:
//   k_pgo_optimize   one resident workgroup of PGO_LANES lanes runs the whole Levenberg-Marquardt loop and, inside it, the preconditioned
//                    conjugate gradients: lane = edge for the residuals, the Jacobian blocks and w_e = J_i p_i + J_j p_j; lane = vertex for
//                    the gathers over the CSR adjacency (edge-index order, no atomics), the 7x7 Cholesky preconditioner and the vector updates.
//                    Every block-wide sum is lane-strided in index order, then the fixed tree over the lanes.
#include "ygz_internal.h"
#include "posemath_dev.h"
#include <cmath>
#include <cstring>
#include <vector>

#define PGO_LANES 256                      // PG_LANES of tests/pgo_ref.c: the lanes of the fixed summation order
#define PGO_CG_CAP 2048                    // bound of the automatic CG cap
#define PG_DMAX 1.7976931348623157e308

namespace {

struct PgoIn {
    double cg_tol, min_rel_decrease;
    int32_t n, ne, max_iterations, max_trials, cg_cap, fix_scale, stage_only, pad;
};

struct PgoDev {
    const PgoIn *in;
    const double *S0;                         // [N][8]
    const uint8_t *fixed;                     // [N]
    const int32_t *edges;                     // [E][2]
    const double *M;                          // [E][8]
    const int32_t *adj_off, *adj;             // [N + 1], [2 E]: 2 e + side per vertex in edge-index order
    // the block that is copied back
    ygz_pgo_result *out;
    double *S;                                // [N][8] the estimate, S_out at the end
    double *res, *Ji, *Jj;                    // [E][7], [E][49], [E][49]
    // work
    double *Sn, *Dg, *Lf, *b, *x, *r, *z, *p, *q, *w;   // [N][8], [N][28], [N][28], 6 x [N][7], [E][7]
};

struct PgoShared {
    double red[PGO_LANES];
    double tot;
};

// ---- the arithmetic (tests/pgo_ref.c, function by function; rotation, Sim3 inverse and retraction, Cholesky loops: posemath_dev.h) ---
__device__ __forceinline__ void pg_compose(const double *A, const double *B, double *out)
{
    double q[4], R[9], r[3];
    ygz_quat_mul(A, B, q);
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    ygz_quat_rotation(A, R);
    ygz_mat3_vec(R, B + 4, r);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[4 + k] = A[7] * r[k] + A[4 + k];
    out[7] = A[7] * B[7];
}

__device__ __forceinline__ int pg_lift(const double *E, double *r)
{
    double x = E[0], y = E[1], z = E[2], w = E[3];
    if (w < 0) { x = -x; y = -y; z = -z; w = -w; }
    if (!(w > 0)) return 0;
    r[0] = 2.0 * x / w; r[1] = 2.0 * y / w; r[2] = 2.0 * z / w;
    r[3] = E[4]; r[4] = E[5]; r[5] = E[6];
    r[6] = 2.0 * (E[7] - 1.0) / (E[7] + 1.0);
    int ok = 1;
#pragma unroll
    for (int k = 0; k < 7; ++k) ok &= fabs(r[k]) <= PG_DMAX;
    return ok;
}

__device__ __forceinline__ int pg_edge_residual(const double *Si, const double *Sj, const double *M, double *E, double *r)
{
    double A[8], Sji[8];
    pg_compose(M, Si, A);
    ygz_sim3_inverse(Sj, Sji);
    pg_compose(A, Sji, E);
    return pg_lift(E, r);
}

// J = sign * L(E) Ad(A), written to global memory row-major
__device__ __forceinline__ void pg_block(const double *E, const double *r, const double *A, double sign, int fix_scale, double *Jout)
{
    double R[9], Lr[9], K[9], J[49];
    ygz_quat_rotation(A, R);
    const double a0 = r[0], a1 = r[1], a2 = r[2];
    Lr[0] = 1.0 + 0.25 * (a0 * a0);       Lr[1] = 0.5 * a2 + 0.25 * (a0 * a1);  Lr[2] = -(0.5 * a1) + 0.25 * (a0 * a2);
    Lr[3] = -(0.5 * a2) + 0.25 * (a1 * a0); Lr[4] = 1.0 + 0.25 * (a1 * a1);     Lr[5] = 0.5 * a0 + 0.25 * (a1 * a2);
    Lr[6] = 0.5 * a1 + 0.25 * (a2 * a0);  Lr[7] = -(0.5 * a0) + 0.25 * (a2 * a1); Lr[8] = 1.0 + 0.25 * (a2 * a2);
    const double d0 = A[4] - E[4], d1 = A[5] - E[5], d2 = A[6] - E[6];
    K[0] = 0.0; K[1] = -d2; K[2] = d1;
    K[3] = d2;  K[4] = 0.0; K[5] = -d0;
    K[6] = -d1; K[7] = d0;  K[8] = 0.0;
    const double c = 4.0 * E[7] / ((E[7] + 1.0) * (E[7] + 1.0));
#pragma unroll
    for (int k = 0; k < 49; ++k) J[k] = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            J[a * 7 + b] = sign * (Lr[3 * a] * R[b] + Lr[3 * a + 1] * R[3 + b] + Lr[3 * a + 2] * R[6 + b]);
            J[(3 + a) * 7 + b] = sign * (K[3 * a] * R[b] + K[3 * a + 1] * R[3 + b] + K[3 * a + 2] * R[6 + b]);
            J[(3 + a) * 7 + 3 + b] = sign * (A[7] * R[3 * a + b]);
        }
    J[3 * 7 + 6] = sign * -d0; J[4 * 7 + 6] = sign * -d1; J[5 * 7 + 6] = sign * -d2;
    J[6 * 7 + 6] = sign * c;
    if (fix_scale)
#pragma unroll
        for (int a = 0; a < 7; ++a) J[a * 7 + 6] = 0.0;
#pragma unroll
    for (int k = 0; k < 49; ++k) Jout[k] = J[k];
}

__device__ __forceinline__ int pg_edge_terms(const double *Si, const double *Sj, const double *M, int fix_scale, double *r, double *Ji, double *Jj)
{
    double E[8];
    const int ok = pg_edge_residual(Si, Sj, M, E, r);
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 7; ++k) r[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 49; ++k) { Ji[k] = 0.0; Jj[k] = 0.0; }
        return 0;
    }
    pg_block(E, r, M, 1.0, fix_scale, Ji);
    pg_block(E, r, E, -1.0, fix_scale, Jj);
    return 1;
}

// D + lambda I, the scale's row and column replaced by the unit ones when the scale is fixed
__device__ __forceinline__ int pg_chol7(const double *D, double lambda, int fix_scale, double *Lo)
{
    double A[49];
    ygz_sym_unpack<7>(D, A);
#pragma unroll
    for (int a = 0; a < 7; ++a) A[a * 7 + a] = A[a * 7 + a] + lambda;
    if (fix_scale) {
#pragma unroll
        for (int a = 0; a < 7; ++a) { A[a * 7 + 6] = 0.0; A[6 * 7 + a] = 0.0; }
        A[48] = 1.0;
    }
    return ygz_chol_factor<7>(A, Lo);
}

// ---- block-wide sums -----------------------------------------------------------------------------------------------------------------
// pg_tree over the lanes' partial sums: strides 128 and 64 out of LDS, 32 .. 1 inside the first wavefront (lane l adds lane l + stride's, the
// same pairs as the tree); two barriers, every lane returns the total
static_assert(PGO_LANES == 256, "pgo_sum spells the tree for 256 lanes");
__device__ __forceinline__ double pgo_sum(PgoShared &sh, double acc)
{
    const int tid = threadIdx.x;
    sh.red[tid] = acc;
    __syncthreads();
    if (tid < 64) {
        double v = (sh.red[tid] + sh.red[tid + 128]) + (sh.red[tid + 64] + sh.red[tid + 192]);
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) v += __shfl_down(v, st);
        if (tid == 0) sh.tot = v;
    }
    __syncthreads();
    return sh.tot;
}

// the largest of the lanes' values (order-free)
__device__ __forceinline__ double pgo_max(PgoShared &sh, double m)
{
    const int tid = threadIdx.x;
    sh.red[tid] = m;
    __syncthreads();
    if (tid < 64) {
        double v = fmax(fmax(sh.red[tid], sh.red[tid + 128]), fmax(sh.red[tid + 64], sh.red[tid + 192]));
#pragma unroll
        for (int st = 32; st >= 1; st >>= 1) v = fmax(v, __shfl_down(v, st));
        if (tid == 0) sh.tot = v;
    }
    __syncthreads();
    return sh.tot;
}

// residuals, both blocks and the cost at D.S (pg_linearize); every lane returns ok, the cost into *cost
__device__ int pgo_linearize(const PgoDev &D, PgoShared &sh, int ne, int fix_scale, double *cost)
{
    __syncthreads();                                                  // S as the vertex lanes last wrote it
    int bad = 0;
    double acc = 0.0;
    for (int e = threadIdx.x; e < ne; e += PGO_LANES) {
        double r[7];
        bad |= !pg_edge_terms(D.S + 8 * D.edges[2 * e], D.S + 8 * D.edges[2 * e + 1], D.M + 8 * (size_t)e, fix_scale, r, D.Ji + 49 * (size_t)e,
                              D.Jj + 49 * (size_t)e);
#pragma unroll
        for (int k = 0; k < 7; ++k) { D.res[7 * (size_t)e + k] = r[k]; acc += r[k] * r[k]; }
    }
    *cost = pgo_sum(sh, acc);
    bad = __syncthreads_or(bad);
    return !bad && fabs(*cost) <= PG_DMAX;
}

// the cost alone at Sx (pg_cost)
__device__ int pgo_cost(const PgoDev &D, PgoShared &sh, const double *Sx, int ne, double *cost)
{
    int bad = 0;
    double acc = 0.0;
    for (int e = threadIdx.x; e < ne; e += PGO_LANES) {
        double E[8], r[7];
        if (!pg_edge_residual(Sx + 8 * D.edges[2 * e], Sx + 8 * D.edges[2 * e + 1], D.M + 8 * (size_t)e, E, r)) { bad = 1; continue; }
#pragma unroll
        for (int k = 0; k < 7; ++k) acc += r[k] * r[k];
    }
    *cost = pgo_sum(sh, acc);
    bad = __syncthreads_or(bad);
    return !bad && fabs(*cost) <= PG_DMAX;
}

// per free vertex: b_v = -sum J^T r, D_v = sum J^T J over its incident edges (pg_gather_system); the largest diagonal element of the lane's
// vertices is returned
__device__ double pgo_gather_system(const PgoDev &D, int n, int fix_scale)
{
    double mx = 0.0;
    for (int v = threadIdx.x; v < n; v += PGO_LANES) {
        if (D.fixed[v]) continue;
        double acc[7], dd[28];
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 28; ++k) dd[k] = 0.0;
        for (int s = D.adj_off[v]; s < D.adj_off[v + 1]; ++s) {
            const int a_ = D.adj[s], e = a_ >> 1;
            const double *Jg = ((a_ & 1) ? D.Jj : D.Ji) + 49 * (size_t)e, *rg = D.res + 7 * (size_t)e;
            double J[49], r[7];
#pragma unroll
            for (int k = 0; k < 49; ++k) J[k] = Jg[k];
#pragma unroll
            for (int k = 0; k < 7; ++k) r[k] = rg[k];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                double t = 0.0;
#pragma unroll
                for (int m = 0; m < 7; ++m) t += J[m * 7 + k] * r[m];
                acc[k] += t;
            }
            int i = 0;
#pragma unroll
            for (int a = 0; a < 7; ++a)
#pragma unroll
                for (int b = a; b < 7; ++b) {
                    double t = 0.0;
#pragma unroll
                    for (int m = 0; m < 7; ++m) t += J[m * 7 + a] * J[m * 7 + b];
                    dd[i++] += t;
                }
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) D.b[7 * v + k] = -acc[k];
        if (fix_scale) D.b[7 * v + 6] = 0.0;
#pragma unroll
        for (int k = 0; k < 28; ++k) D.Dg[28 * v + k] = dd[k];
        int m = 0;
#pragma unroll
        for (int a = 0; a < 7; ++a) { const double h = fabs(dd[m]); if (h > mx) mx = h; m += 7 - a; }
    }
    return mx;
}

// preconditioned CG from x = 0 (pg_cg): every lane runs the same control flow on the block-wide sums; returns the iterations run
__device__ int pgo_cg(const PgoDev &D, PgoShared &sh, int n, int ne, int fix_scale, double lambda, double tol, int cap, int *capped)
{
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int v = tid; v < n; v += PGO_LANES) {
        if (D.fixed[v]) continue;
        double r[7], z[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) { r[k] = D.b[7 * v + k]; D.x[7 * v + k] = 0.0; D.r[7 * v + k] = r[k]; }
        ygz_chol_solve_packed<7>(D.Lf + 28 * v, r, z);
#pragma unroll
        for (int k = 0; k < 7; ++k) { D.z[7 * v + k] = z[k]; D.p[7 * v + k] = z[k]; acc += r[k] * z[k]; }
    }
    double rz = pgo_sum(sh, acc);                                     // its barriers also publish p
    const double stop = (tol * tol) * rz;
    int it = 0;
    *capped = 0;
    for (;;) {
        if (rz <= stop) break;
        if (it >= cap) { *capped = 1; break; }
        // lane = edge: w_e = J_i p_i + J_j p_j
        for (int e = tid; e < ne; e += PGO_LANES) {
            const int i = D.edges[2 * e], j = D.edges[2 * e + 1];
            const int fi = D.fixed[i], fj = D.fixed[j];
            const double *Ji = D.Ji + 49 * (size_t)e, *Jj = D.Jj + 49 * (size_t)e;
            double pi[7], pj[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) { pi[k] = fi ? 0.0 : D.p[7 * i + k]; pj[k] = fj ? 0.0 : D.p[7 * j + k]; }
#pragma unroll
            for (int m = 0; m < 7; ++m) {
                double t = 0.0;
                if (!fi)
#pragma unroll
                    for (int k = 0; k < 7; ++k) t += Ji[m * 7 + k] * pi[k];
                if (!fj)
#pragma unroll
                    for (int k = 0; k < 7; ++k) t += Jj[m * 7 + k] * pj[k];
                D.w[7 * (size_t)e + m] = t;
            }
        }
        __syncthreads();
        // lane = vertex: q_v = sum J^T w + lambda p_v, and the lane's part of p . q
        acc = 0.0;
        for (int v = tid; v < n; v += PGO_LANES) {
            if (D.fixed[v]) continue;
            double g[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) g[k] = 0.0;
            for (int s = D.adj_off[v]; s < D.adj_off[v + 1]; ++s) {
                const int a_ = D.adj[s], e = a_ >> 1;
                const double *J = ((a_ & 1) ? D.Jj : D.Ji) + 49 * (size_t)e, *wg = D.w + 7 * (size_t)e;
                double w[7];
#pragma unroll
                for (int m = 0; m < 7; ++m) w[m] = wg[m];
#pragma unroll
                for (int k = 0; k < 7; ++k) {
                    double t = 0.0;
#pragma unroll
                    for (int m = 0; m < 7; ++m) t += J[m * 7 + k] * w[m];
                    g[k] += t;
                }
            }
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const double pk = D.p[7 * v + k];
                double qk = g[k] + lambda * pk;
                if (fix_scale && k == 6) qk = pk;
                D.q[7 * v + k] = qk;
                acc += pk * qk;
            }
        }
        const double pq = pgo_sum(sh, acc);
        if (!(pq > 0)) break;
        const double alpha = rz / pq;
        acc = 0.0;
        for (int v = tid; v < n; v += PGO_LANES) {
            if (D.fixed[v]) continue;
            double r[7], z[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                D.x[7 * v + k] = D.x[7 * v + k] + alpha * D.p[7 * v + k];
                r[k] = D.r[7 * v + k] - alpha * D.q[7 * v + k];
                D.r[7 * v + k] = r[k];
            }
            ygz_chol_solve_packed<7>(D.Lf + 28 * v, r, z);
#pragma unroll
            for (int k = 0; k < 7; ++k) { D.z[7 * v + k] = z[k]; acc += r[k] * z[k]; }
        }
        const double rzn = pgo_sum(sh, acc);
        const double beta = rzn / rz;
        for (int v = tid; v < n; v += PGO_LANES) {
            if (D.fixed[v]) continue;
#pragma unroll
            for (int k = 0; k < 7; ++k) D.p[7 * v + k] = D.z[7 * v + k] + beta * D.p[7 * v + k];
        }
        rz = rzn;
        ++it;
        __syncthreads();                                              // p for the edge lanes
    }
    return it;
}

__global__ __launch_bounds__(PGO_LANES) void k_pgo_optimize(PgoDev D)
{
    __shared__ PgoShared sh;
    const int tid = threadIdx.x;
    const PgoIn &in = *D.in;
    const int n = in.n, ne = in.ne, fix_scale = in.fix_scale, cap = in.cg_cap;
    for (int k = tid; k < 8 * n; k += PGO_LANES) D.S[k] = D.S0[k];
    ygz_pgo_result o;
    o.cost_initial = 0.0; o.cost_final = 0.0; o.lambda = 0.0;
    o.status = YGZ_PGO_MAX_ITERATIONS; o.lm_iterations = 0; o.n_solves = 0; o.cg_iterations_total = 0; o.cg_capped = 0; o.pad = 0;
    if (in.stage_only) {
        double cost;
        const int ok = pgo_linearize(D, sh, ne, fix_scale, &cost);
        o.cost_initial = cost; o.cost_final = cost; o.status = ok ? YGZ_PGO_MAX_ITERATIONS : YGZ_PGO_FAILED;
        if (tid == 0) *D.out = o;
        return;
    }
    double lambda = 0.0, ni = 2.0, currentChi = 0.0;
    int status = YGZ_PGO_MAX_ITERATIONS;
    for (int it = 0; it < in.max_iterations; ++it) {
        double cost;
        const int lin_ok = pgo_linearize(D, sh, ne, fix_scale, &cost);
        if (it == 0) {
            if (!lin_ok) { status = YGZ_PGO_FAILED; break; }
            o.cost_initial = cost;
        }
        currentChi = cost;
        const double lane_mx = pgo_gather_system(D, n, fix_scale);
        if (it == 0) {
            const double mx = pgo_max(sh, lane_mx);
            lambda = 1e-5 * mx; ni = 2.0;
        }
        double rho = 0.0;
        int qmax = 0, converged = 0;
        do {
            int bad = 0;
            for (int v = tid; v < n; v += PGO_LANES)
                if (!D.fixed[v]) bad |= !pg_chol7(D.Dg + 28 * v, lambda, fix_scale, D.Lf + 28 * v);
            int ok = !__syncthreads_or(bad);
            double tempChi = PG_DMAX;
            if (ok) {
                int capped = 0;
                o.cg_iterations_total += pgo_cg(D, sh, n, ne, fix_scale, lambda, in.cg_tol, cap, &capped);
                o.cg_capped += capped;
                ++o.n_solves;
                bad = 0;
                for (int v = tid; v < n; v += PGO_LANES) {
                    double S[8], x[7], Sn[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) S[k] = D.S[8 * v + k];
                    int zero = 1;
                    const int fx = D.fixed[v];
                    if (!fx)
#pragma unroll
                        for (int k = 0; k < 7; ++k) { x[k] = D.x[7 * v + k]; zero &= x[k] == 0.0; }
                    if (fx || zero) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) Sn[k] = S[k];
                    } else if (!ygz_sim3_retract(S, x, Sn)) {
                        bad = 1;
#pragma unroll
                        for (int k = 0; k < 8; ++k) Sn[k] = S[k];
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) D.Sn[8 * v + k] = Sn[k];
                }
                ok = !__syncthreads_or(bad);                          // also publishes Sn
            }
            if (ok) {
                ok = pgo_cost(D, sh, D.Sn, ne, &tempChi);
                if (!ok) tempChi = PG_DMAX;
            }
            rho = currentChi - tempChi;
            double scale = 0.0;
            if (ok) {
                double acc = 0.0;
                for (int v = tid; v < n; v += PGO_LANES) {
                    if (D.fixed[v]) continue;
#pragma unroll
                    for (int k = 0; k < 7; ++k) { const double xk = D.x[7 * v + k]; acc += xk * (lambda * xk + D.b[7 * v + k]); }
                }
                scale = pgo_sum(sh, acc);
            }
            scale += 1e-3;
            rho = rho / scale;
            if (ok && rho > 0 && fabs(tempChi) <= PG_DMAX) {
                const double u = 2.0 * rho - 1.0;
                double alpha = 1.0 - u * u * u;
                if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                lambda = lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
                ni = 2.0;
                converged = currentChi - tempChi <= in.min_rel_decrease * currentChi;
                currentChi = tempChi;
                for (int k = tid; k < 8 * n; k += PGO_LANES) D.S[k] = D.Sn[k];     // pgo_linearize starts with a barrier
            } else {
                lambda = lambda * ni; ni = ni * 2.0;
                if (!(fabs(lambda) <= PG_DMAX)) break;
            }
            ++qmax;
        } while (rho < 0 && qmax < in.max_trials);
        ++o.lm_iterations;
        if (qmax == in.max_trials || rho == 0 || !(fabs(lambda) <= PG_DMAX)) { status = YGZ_PGO_STALLED; break; }
        if (converged) { status = YGZ_PGO_CONVERGED; break; }
    }
    o.status = status;
    o.cost_final = status == YGZ_PGO_FAILED ? 0.0 : currentChi;
    o.lambda = lambda;
    if (tid == 0) *D.out = o;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
bool finite8(const double *v)
{
    for (int k = 0; k < 8; ++k) if (!(std::fabs(v[k]) <= PG_DMAX)) return false;
    return true;
}

// every refusal of the header, in its order, before anything touches the device
int validate(const ygz_hip_ctx *ctx, int n, const double *S, const uint8_t *fixed, int ne, const int32_t *edges, const double *M,
             const ygz_pgo_params &p)
{
    if (!S || !fixed || !edges || !M) return YGZ_E_INVALID;
    if (n > YGZ_PGO_MAX_VERTICES || ne > YGZ_PGO_MAX_EDGES) return YGZ_E_CAPACITY;
    if (n < 2 || ne < 1) return YGZ_E_INVALID;
    if (p.max_iterations < 1 || p.max_iterations > 1000 || p.max_trials < 1 || p.max_trials > 100 || p.cg_max_iterations < 0
        || p.cg_max_iterations > 65536 || !(p.cg_tol > 0 && p.cg_tol < 1) || !(p.min_rel_decrease >= 0 && p.min_rel_decrease < 1))
        return YGZ_E_INVALID;
    std::vector<char> has(n, 0);
    for (int e = 0; e < ne; ++e) {
        const int i = edges[2 * e], j = edges[2 * e + 1];
        if (i < 0 || i >= n || j < 0 || j >= n || i == j) return YGZ_E_INVALID;
        has[i] = has[j] = 1;
        if (!finite8(M + 8 * (size_t)e) || !(M[8 * (size_t)e + 7] > 0)) return YGZ_E_INVALID;
    }
    int n_free = 0;
    for (int v = 0; v < n; ++v) {
        if (!finite8(S + 8 * (size_t)v) || !(S[8 * (size_t)v + 7] > 0)) return YGZ_E_INVALID;
        if (fixed[v]) continue;
        ++n_free;
        if (!has[v]) return YGZ_E_INVALID;
    }
    if (n_free < 1) return YGZ_E_INVALID;
    if (!ctx) return YGZ_E_INVALID;
    return YGZ_OK;
}

struct Layout {
    size_t in, s0, fixed, edges, m, adj_off, adj, in_end;             // the upload
    size_t out, s, out_end, res, ji, jj, stage_end;                   // the copy back: [out, out_end) or [out, stage_end)
    size_t sn, dg, lf, vec, w, total;                                 // work
};
Layout layout(size_t N, size_t E)
{
    Layout L;
    YgzBlobLayout B;
    L.in = B.add(sizeof(PgoIn));
    L.s0 = B.add_n<double>(N * 8);
    L.fixed = B.add(N);
    L.edges = B.add_n<int32_t>(E * 2);
    L.m = B.add_n<double>(E * 8);
    L.adj_off = B.add_n<int32_t>(N + 1);
    L.adj = B.add_n<int32_t>(E * 2);
    L.in_end = B.end;
    L.out = B.add(sizeof(ygz_pgo_result));
    L.s = B.add_n<double>(N * 8);
    L.out_end = B.end;
    L.res = B.add_n<double>(E * 7);
    L.ji = B.add_n<double>(E * 49);
    L.jj = B.add_n<double>(E * 49);
    L.stage_end = B.end;
    L.sn = B.add_n<double>(N * 8);
    L.dg = B.add_n<double>(N * 28);
    L.lf = B.add_n<double>(N * 28);
    L.vec = B.add(6 * ygz_round_up_256(N * 56));             // b, x, r, z, p, q: [N][7] each, 256-aligned
    L.w = B.add_n<double>(E * 7);
    L.total = B.end;
    return L;
}

// validation, the adjacency, one upload, the launch, one copy back of [out, out_end) (stage = false) or of [out, stage_end), one wait; `down`
// receives the page-locked image of the block
int run(ygz_hip_ctx *ctx, int n, const double *S, const uint8_t *fixed, int ne, const int32_t *edges, const double *M,
        const ygz_pgo_params *params, bool stage, uint8_t **down, Layout *Lout)
{
    ygz_pgo_params p;
    if (params) p = *params; else ygz_hip_default_pgo_params(&p);
    const int rv = validate(ctx, n, S, fixed, ne, edges, M, p);
    if (rv != YGZ_OK) return rv;
    YgzDeviceGuard dg_(ctx);
    { int rj_ = ygz_join(ctx); if (rj_ != YGZ_OK) return rj_; }
    const size_t N = (size_t)n, E = (size_t)ne;
    const Layout L = layout(N, E);
    const size_t down_end = stage ? L.stage_end : L.out_end;  // [0, in_end) goes up, [out, down_end) comes back
    YgzBlob b;
    int rc = ygz_blob_open(ctx, SCR_PGO, L.total, down_end, &b);
    if (rc != YGZ_OK) return rc;
    uint8_t *up = b.host, *dev = b.dev;
    PgoIn in;
    memset(&in, 0, sizeof in);
    int n_free = 0;
    for (int v = 0; v < n; ++v) n_free += !fixed[v];
    in.cg_tol = p.cg_tol; in.min_rel_decrease = p.min_rel_decrease; in.n = n; in.ne = ne; in.max_iterations = p.max_iterations;
    in.max_trials = p.max_trials; in.fix_scale = p.fix_scale != 0; in.stage_only = stage ? 1 : 0;
    in.cg_cap = p.cg_max_iterations > 0 ? p.cg_max_iterations : (7 * n_free < PGO_CG_CAP ? 7 * n_free : PGO_CG_CAP);
    memcpy(up + L.in, &in, sizeof in);
    memcpy(up + L.s0, S, N * 64);
    for (int v = 0; v < n; ++v) up[L.fixed + v] = fixed[v] ? 1 : 0;
    memcpy(up + L.edges, edges, E * 8);
    memcpy(up + L.m, M, E * 64);
    // the CSR adjacency (pg_adjacency): per vertex its edges in edge-index order
    int32_t *adj_off = ygz_at<int32_t>(up, L.adj_off), *adj = ygz_at<int32_t>(up, L.adj);
    for (int v = 0; v <= n; ++v) adj_off[v] = 0;
    for (int e = 0; e < ne; ++e) { ++adj_off[edges[2 * e] + 1]; ++adj_off[edges[2 * e + 1] + 1]; }
    for (int v = 0; v < n; ++v) adj_off[v + 1] += adj_off[v];
    std::vector<int32_t> fill(adj_off, adj_off + n);
    for (int e = 0; e < ne; ++e) { adj[fill[edges[2 * e]]++] = 2 * e; adj[fill[edges[2 * e + 1]]++] = 2 * e + 1; }
    if ((rc = ygz_blob_upload(ctx, b, L.in_end)) != YGZ_OK) return rc;
    PgoDev D;
    D.in = ygz_at<const PgoIn>(dev, L.in); D.S0 = ygz_at<const double>(dev, L.s0); D.fixed = dev + L.fixed;
    D.edges = ygz_at<const int32_t>(dev, L.edges); D.M = ygz_at<const double>(dev, L.m);
    D.adj_off = ygz_at<const int32_t>(dev, L.adj_off); D.adj = ygz_at<const int32_t>(dev, L.adj);
    D.out = ygz_at<ygz_pgo_result>(dev, L.out); D.S = ygz_at<double>(dev, L.s);
    D.res = ygz_at<double>(dev, L.res); D.Ji = ygz_at<double>(dev, L.ji); D.Jj = ygz_at<double>(dev, L.jj);
    D.Sn = ygz_at<double>(dev, L.sn); D.Dg = ygz_at<double>(dev, L.dg); D.Lf = ygz_at<double>(dev, L.lf);
    const size_t vs = ygz_round_up_256(N * 56);
    D.b = ygz_at<double>(dev, L.vec); D.x = ygz_at<double>(dev, L.vec + vs); D.r = ygz_at<double>(dev, L.vec + 2 * vs);
    D.z = ygz_at<double>(dev, L.vec + 3 * vs); D.p = ygz_at<double>(dev, L.vec + 4 * vs); D.q = ygz_at<double>(dev, L.vec + 5 * vs);
    D.w = ygz_at<double>(dev, L.w);
    YGZ_LAUNCH(ctx, KID_COUNT, k_pgo_optimize, dim3(1), dim3(PGO_LANES), D);
    if ((rc = ygz_blob_fetch(ctx, b, L.out, down_end)) != YGZ_OK) return rc;
    *down = up;
    *Lout = L;
    return YGZ_OK;
}

}  // namespace

extern "C" {

void ygz_hip_default_pgo_params(ygz_pgo_params *p)
{
    if (!p) return;
    p->max_iterations = 20; p->max_trials = 10; p->cg_max_iterations = 0; p->fix_scale = 0;
    p->cg_tol = 1e-8; p->min_rel_decrease = 1e-9;
}

int ygz_hip_pose_graph_optimize(ygz_hip_ctx *ctx, int n_vertices, const double *S, const uint8_t *fixed, int n_edges, const int32_t *edges,
                                const double *M, const ygz_pgo_params *params, double *S_out, ygz_pgo_result *result)
{
    if (!S_out || !result) return YGZ_E_INVALID;
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, n_vertices, S, fixed, n_edges, edges, M, params, false, &o, &L);
    if (rc != YGZ_OK) return rc;
    memcpy(result, o + L.out, sizeof(ygz_pgo_result));
    memcpy(S_out, result->status == YGZ_PGO_FAILED ? (const void *)S : (const void *)(o + L.s), (size_t)n_vertices * 64);
    return YGZ_OK;
}

int ygz_hip_pgo_linearize(ygz_hip_ctx *ctx, int n_vertices, const double *S, const uint8_t *fixed, int n_edges, const int32_t *edges,
                          const double *M, const ygz_pgo_params *params, double *residuals, double *Ji, double *Jj, double *cost)
{
    uint8_t *o = nullptr;
    Layout L;
    const int rc = run(ctx, n_vertices, S, fixed, n_edges, edges, M, params, true, &o, &L);
    if (rc != YGZ_OK) return rc;
    const ygz_pgo_result *r = ygz_at<const ygz_pgo_result>(o, L.out);
    const size_t E = (size_t)n_edges;
    if (residuals) memcpy(residuals, o + L.res, E * 56);
    if (Ji) memcpy(Ji, o + L.ji, E * 392);
    if (Jj) memcpy(Jj, o + L.jj, E * 392);
    if (cost) *cost = r->cost_initial;
    return r->status == YGZ_PGO_FAILED ? YGZ_E_STATE : YGZ_OK;
}

}  // extern "C"
