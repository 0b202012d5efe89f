/* pgo_ref.c -- restatement of the Sim3 pose-graph optimiser (ygz_slam_amd/csrc/pgo.hip): the yardstick of tests/test_pgo_ref.py and
 * tests/test_gpu_pgo.py, and the frozen spec of DESIGN.md section 13.  What ORB-SLAM2's Optimizer::OptimizeEssentialGraph leaves to g2o
 * and Eigen is stated here function by function in the kernel's operation order.  Test infrastructure: plain C99, single-threaded, built
 * by tests/pgo_ref.py with -O2 -ffp-contract=off -fno-fast-math, never linked into the product.  Only + - * / and sqrt.
 *
 *  - a vertex is a similarity S_i (world -> camera i) stored qx qy qz qw tx ty tz s; an edge (i, j) carries M_ji ~ S_j o S_i^-1;
 *  - residual r_e = lift(M_ji o S_i o S_j^-1), seven numbers; the information matrix is the identity;
 *  - retraction S_i <- Delta(d_i) o S_i, sim3_ref.c's update; a vertex whose step is exactly zero keeps its bits;
 *  - Jacobians exact at the linearisation point: J_i = L(E) Ad(M), J_j = -L(E) Ad(E), E = M o S_i o S_j^-1;
 *  - outer loop: Levenberg-Marquardt with g2o's rules (sim3_ref.c's sr_lm) and a relative-decrease stop;
 *  - inner solve: preconditioned conjugate gradients on (H + lambda I) d = b over the free vertices, H = J^T J never assembled, the
 *    preconditioner the inverse of every vertex's 7x7 diagonal block plus lambda (Cholesky);
 *  - every sum over vertices or edges is lane-strided over PG_LANES lanes in index order, then a fixed tree over the lanes; every sum
 *    over a vertex's incident edges runs in edge-index order (a CSR adjacency). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define PG_LANES 256           /* lanes of k_pgo_optimize */
#define PG_DMAX 1.7976931348623157e308
#define PG_CG_CAP 2048         /* bound of the automatic CG cap */

enum { PG_FAILED = 0, PG_CONVERGED = 1, PG_MAX_ITERATIONS = 2, PG_STALLED = 3 };

/* the layouts of ygz_pgo_params and ygz_pgo_result (include/ygz_hip.h) */
typedef struct {
    int32_t max_iterations, max_trials, cg_max_iterations, fix_scale;
    double  cg_tol, min_rel_decrease;
} pg_params;

typedef struct {
    double  cost_initial, cost_final, lambda;
    int32_t status, lm_iterations, n_solves, cg_iterations_total, cg_capped, pad;
} pg_result;

/* ---- Sim3 algebra ------------------------------------------------------------------------------------------------------------ */
/* on the device: ygz_quat_rotation (ygz_slam_amd/csrc/posemath_dev.h) */
void pg_rotation(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

/* on the device: ygz_mat3_vec (ygz_slam_amd/csrc/posemath_dev.h) */
static void mat_vec(const double *R, const double *v, double *o)
{
    for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
}

/* S^-1: (1/s, R^T, -(1/s) R^T t) */
/* on the device: ygz_sim3_inverse (ygz_slam_amd/csrc/posemath_dev.h) */
void pg_inverse(const double *S, double *Si)
{
    Si[0] = -S[0]; Si[1] = -S[1]; Si[2] = -S[2]; Si[3] = S[3];
    Si[7] = 1.0 / S[7];
    double R[9], r[3];
    pg_rotation(Si, R);
    mat_vec(R, S + 4, r);
    for (int k = 0; k < 3; ++k) Si[4 + k] = -(Si[7] * r[k]);
}

/* A o B: (qA qB normalised, sA RA tB + tA, sA sB) */
void pg_compose(const double *A, const double *B, double *out)
{
    const double ax = A[0], ay = A[1], az = A[2], aw = A[3], bx = B[0], by = B[1], bz = B[2], bw = B[3];
    double q[4];
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by - ax * bz + ay * bw + az * bx;
    q[2] = aw * bz + ax * by - ay * bx + az * bw;
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    double R[9], r[3];
    pg_rotation(A, R);
    mat_vec(R, B + 4, r);
    for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
    for (int k = 0; k < 3; ++k) out[4 + k] = A[7] * r[k] + A[4 + k];
    out[7] = A[7] * B[7];
}

/* the left-multiplicative update S <- Delta(x) o S, x = (omega, t, sigma): sim3_ref.c's sr_apply_delta; 0 when |sigma| >= 2 */
/* on the device: ygz_sim3_retract (ygz_slam_amd/csrc/posemath_dev.h) */
int pg_retract(const double *S, const double *x, double *out)
{
    if (!(fabs(x[6]) < 2.0)) return 0;
    double dq[4] = { 0.5 * x[0], 0.5 * x[1], 0.5 * x[2], 1.0 };
    const double dn = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    for (int k = 0; k < 4; ++k) dq[k] = dq[k] / dn;
    const double ds = (2.0 + x[6]) / (2.0 - x[6]);
    const double ax = dq[0], ay = dq[1], az = dq[2], aw = dq[3], bx = S[0], by = S[1], bz = S[2], bw = S[3];
    double q[4];
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by - ax * bz + ay * bw + az * bx;
    q[2] = aw * bz + ax * by - ay * bx + az * bw;
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
    double dR[9], r[3];
    pg_rotation(dq, dR);
    mat_vec(dR, S + 4, r);
    for (int k = 0; k < 3; ++k) out[4 + k] = ds * r[k] + x[3 + k];
    out[7] = ds * S[7];
    return 1;
}

/* the inverse of Delta: (2 q_v / w, t, 2 (s - 1) / (s + 1)) with the sign of q chosen so that w >= 0; 0 when w <= 0 after that (a
 * rotation of 180 degrees) or a value is not finite */
int pg_lift(const double *E, double *r)
{
    double x = E[0], y = E[1], z = E[2], w = E[3];
    if (w < 0) { x = -x; y = -y; z = -z; w = -w; }
    if (!(w > 0)) return 0;
    r[0] = 2.0 * x / w; r[1] = 2.0 * y / w; r[2] = 2.0 * z / w;
    r[3] = E[4]; r[4] = E[5]; r[5] = E[6];
    r[6] = 2.0 * (E[7] - 1.0) / (E[7] + 1.0);
    int ok = 1;
    for (int k = 0; k < 7; ++k) ok &= fabs(r[k]) <= PG_DMAX;
    return ok;
}

/* E = M o S_i o S_j^-1 and r = lift(E) */
int pg_edge_residual(const double *Si, const double *Sj, const double *M, double *E, double *r)
{
    double A[8], Sji[8];
    pg_compose(M, Si, A);
    pg_inverse(Sj, Sji);
    pg_compose(A, Sji, E);
    return pg_lift(E, r);
}

/* J = sign * L(E) Ad(A), 7x7 row-major: with a = r[0..2], t0 = E's translation, (R, t, s) = A's
 *   rows 0-2: [ (I - [a]x / 2 + a a^T / 4) R, 0, 0 ]      rows 3-5: [ [t - t0]x R, s R, t0 - t ]      row 6: [ 0, 0, 4 s0 / (s0 + 1)^2 ] */
static void pg_block(const double *E, const double *r, const double *A, double sign, int fix_scale, double *J)
{
    double R[9], Lr[9], K[9];
    pg_rotation(A, R);
    const double a0 = r[0], a1 = r[1], a2 = r[2];
    Lr[0] = 1.0 + 0.25 * (a0 * a0);       Lr[1] = 0.5 * a2 + 0.25 * (a0 * a1);  Lr[2] = -(0.5 * a1) + 0.25 * (a0 * a2);
    Lr[3] = -(0.5 * a2) + 0.25 * (a1 * a0); Lr[4] = 1.0 + 0.25 * (a1 * a1);     Lr[5] = 0.5 * a0 + 0.25 * (a1 * a2);
    Lr[6] = 0.5 * a1 + 0.25 * (a2 * a0);  Lr[7] = -(0.5 * a0) + 0.25 * (a2 * a1); Lr[8] = 1.0 + 0.25 * (a2 * a2);
    const double d0 = A[4] - E[4], d1 = A[5] - E[5], d2 = A[6] - E[6];
    K[0] = 0.0; K[1] = -d2; K[2] = d1;
    K[3] = d2;  K[4] = 0.0; K[5] = -d0;
    K[6] = -d1; K[7] = d0;  K[8] = 0.0;
    const double c = 4.0 * E[7] / ((E[7] + 1.0) * (E[7] + 1.0));
    for (int k = 0; k < 49; ++k) J[k] = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            J[a * 7 + b] = sign * (Lr[3 * a] * R[b] + Lr[3 * a + 1] * R[3 + b] + Lr[3 * a + 2] * R[6 + b]);
            J[(3 + a) * 7 + b] = sign * (K[3 * a] * R[b] + K[3 * a + 1] * R[3 + b] + K[3 * a + 2] * R[6 + b]);
            J[(3 + a) * 7 + 3 + b] = sign * (A[7] * R[3 * a + b]);
        }
    J[3 * 7 + 6] = sign * -d0; J[4 * 7 + 6] = sign * -d1; J[5 * 7 + 6] = sign * -d2;
    J[6 * 7 + 6] = sign * c;
    if (fix_scale)
        for (int a = 0; a < 7; ++a) J[a * 7 + 6] = 0.0;
}

/* residual and both Jacobian blocks of one edge: dr/dd_i (Ji) and dr/dd_j (Jj); 0 when the residual is rejected */
int pg_edge_terms(const double *Si, const double *Sj, const double *M, int fix_scale, double *r, double *Ji, double *Jj)
{
    double E[8];
    const int ok = pg_edge_residual(Si, Sj, M, E, r);
    if (!ok) {
        for (int k = 0; k < 7; ++k) r[k] = 0.0;
        for (int k = 0; k < 49; ++k) { Ji[k] = 0.0; Jj[k] = 0.0; }
        return 0;
    }
    pg_block(E, r, M, 1.0, fix_scale, Ji);
    pg_block(E, r, E, -1.0, fix_scale, Jj);
    return 1;
}

/* ---- 7x7 Cholesky of a diagonal block ------------------------------------------------------------------------------------------ */
/* D: the upper triangle row by row (28); L: the factor of D + lambda I, lower triangle row by row (28); with fix_scale row and column 6
 * are the identity's; 0 on a non-positive pivot */
/* on the device: pg_chol7 of pgo.hip on ygz_sym_unpack and ygz_chol_factor (ygz_slam_amd/csrc/posemath_dev.h) */
int pg_chol7(const double *D, double lambda, int fix_scale, double *Lo)
{
    double A[49], L[49];
    int m = 0;
    for (int a = 0; a < 7; ++a)
        for (int b = a; b < 7; ++b) { A[a * 7 + b] = D[m]; A[b * 7 + a] = D[m]; ++m; }
    for (int a = 0; a < 7; ++a) A[a * 7 + a] = A[a * 7 + a] + lambda;
    if (fix_scale) {
        for (int a = 0; a < 7; ++a) { A[a * 7 + 6] = 0.0; A[6 * 7 + a] = 0.0; }
        A[48] = 1.0;
    }
    for (int k = 0; k < 49; ++k) L[k] = 0.0;
    int ok = 1;
    for (int j = 0; j < 7; ++j) {
        double d = A[j * 7 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 7 + k] * L[j * 7 + k];
        ok &= d > 0;
        const double ljj = sqrt(d);
        L[j * 7 + j] = ljj;
        for (int i = j + 1; i < 7; ++i) {
            double v = A[i * 7 + j];
            for (int k = 0; k < j; ++k) v -= L[i * 7 + k] * L[j * 7 + k];
            L[i * 7 + j] = v / ljj;
        }
    }
    m = 0;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j <= i; ++j) Lo[m++] = L[i * 7 + j];
    return ok;
}

/* x = (L L^T)^-1 b */
/* on the device: ygz_chol_solve_packed (ygz_slam_amd/csrc/posemath_dev.h) */
void pg_chol7_solve(const double *Lo, const double *b, double *x)
{
    double L[49], y[7];
    int m = 0;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j <= i; ++j) L[i * 7 + j] = Lo[m++];
    for (int i = 0; i < 7; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= L[i * 7 + k] * y[k];
        y[i] = v / L[i * 7 + i];
    }
    for (int i = 6; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 7; ++k) v -= L[k * 7 + i] * x[k];
        x[i] = v / L[i * 7 + i];
    }
}

/* ---- block-wide sums ----------------------------------------------------------------------------------------------------------- */
static double pg_tree(double *lane)
{
    for (int st = PG_LANES / 2; st >= 1; st /= 2)
        for (int l = 0; l < st; ++l) lane[l] += lane[l + st];
    return lane[0];
}

/* sum over the free vertices of a_v . b_v */
static double pg_dot(const double *a, const double *b, const uint8_t *fixed, int n)
{
    double lane[PG_LANES];
    for (int l = 0; l < PG_LANES; ++l) {
        double acc = 0.0;
        for (int v = l; v < n; v += PG_LANES) {
            if (fixed[v]) continue;
            for (int k = 0; k < 7; ++k) acc += a[7 * v + k] * b[7 * v + k];
        }
        lane[l] = acc;
    }
    return pg_tree(lane);
}

/* the adjacency: adj_off [N + 1], adj [2 E] = 2 e + side (0: the vertex is the edge's i, 1: its j), per vertex in edge-index order */
void pg_adjacency(int n, int ne, const int32_t *edges, int32_t *adj_off, int32_t *adj)
{
    for (int v = 0; v <= n; ++v) adj_off[v] = 0;
    for (int e = 0; e < ne; ++e) { ++adj_off[edges[2 * e] + 1]; ++adj_off[edges[2 * e + 1] + 1]; }
    for (int v = 0; v < n; ++v) adj_off[v + 1] += adj_off[v];
    int32_t *fill = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    for (int v = 0; v < n; ++v) fill[v] = adj_off[v];
    for (int e = 0; e < ne; ++e) { adj[fill[edges[2 * e]]++] = 2 * e; adj[fill[edges[2 * e + 1]]++] = 2 * e + 1; }
    free(fill);
}

/* residuals [E][7], both blocks [E][49] each and the cost at S; 0 when an edge's residual is rejected (its terms are zero then) */
int pg_linearize(int n, const double *S, int ne, const int32_t *edges, const double *M, int fix_scale, double *res, double *Ji, double *Jj,
                 double *cost)
{
    double lane[PG_LANES];
    int ok = 1;
    (void)n;
    for (int l = 0; l < PG_LANES; ++l) {
        double acc = 0.0;
        for (int e = l; e < ne; e += PG_LANES) {
            ok &= pg_edge_terms(S + 8 * edges[2 * e], S + 8 * edges[2 * e + 1], M + 8 * e, fix_scale, res + 7 * e, Ji + 49 * e, Jj + 49 * e);
            for (int k = 0; k < 7; ++k) acc += res[7 * e + k] * res[7 * e + k];
        }
        lane[l] = acc;
    }
    *cost = pg_tree(lane);
    return ok && fabs(*cost) <= PG_DMAX;
}

/* the cost alone at S */
static int pg_cost(const double *S, int ne, const int32_t *edges, const double *M, double *cost)
{
    double lane[PG_LANES];
    int ok = 1;
    for (int l = 0; l < PG_LANES; ++l) {
        double acc = 0.0;
        for (int e = l; e < ne; e += PG_LANES) {
            double E[8], r[7];
            if (!pg_edge_residual(S + 8 * edges[2 * e], S + 8 * edges[2 * e + 1], M + 8 * e, E, r)) { ok = 0; continue; }
            for (int k = 0; k < 7; ++k) acc += r[k] * r[k];
        }
        lane[l] = acc;
    }
    *cost = pg_tree(lane);
    return ok && fabs(*cost) <= PG_DMAX;
}

typedef struct {
    int n, ne, fix_scale;
    const uint8_t *fixed;
    const int32_t *edges, *adj_off, *adj;
    double *Ji, *Jj, *res, *D, *b, *Lf, *x, *r, *z, *p, *q, *w;
} pg_work;

/* per free vertex: b_v = -sum J^T r and D_v = sum J^T J (upper triangle) over its incident edges */
static void pg_gather_system(const pg_work *W)
{
    for (int v = 0; v < W->n; ++v) {
        if (W->fixed[v]) continue;
        double acc[7], dd[28];
        for (int k = 0; k < 7; ++k) acc[k] = 0.0;
        for (int k = 0; k < 28; ++k) dd[k] = 0.0;
        for (int s = W->adj_off[v]; s < W->adj_off[v + 1]; ++s) {
            const int e = W->adj[s] >> 1;
            const double *J = ((W->adj[s] & 1) ? W->Jj : W->Ji) + 49 * (size_t)e, *r = W->res + 7 * (size_t)e;
            for (int k = 0; k < 7; ++k) {
                double t = 0.0;
                for (int m = 0; m < 7; ++m) t += J[m * 7 + k] * r[m];
                acc[k] += t;
            }
            int i = 0;
            for (int a = 0; a < 7; ++a)
                for (int b = a; b < 7; ++b) {
                    double t = 0.0;
                    for (int m = 0; m < 7; ++m) t += J[m * 7 + a] * J[m * 7 + b];
                    dd[i++] += t;
                }
        }
        for (int k = 0; k < 7; ++k) W->b[7 * v + k] = -acc[k];
        if (W->fix_scale) W->b[7 * v + 6] = 0.0;
        for (int k = 0; k < 28; ++k) W->D[28 * v + k] = dd[k];
    }
}

/* q = (H + lambda I) p over the free vertices: w_e = J_i p_i + J_j p_j per edge, then the gather per vertex */
static void pg_apply(const pg_work *W, double lambda)
{
    for (int e = 0; e < W->ne; ++e) {
        const int i = W->edges[2 * e], j = W->edges[2 * e + 1];
        const double *Ji = W->Ji + 49 * (size_t)e, *Jj = W->Jj + 49 * (size_t)e;
        for (int m = 0; m < 7; ++m) {
            double t = 0.0;
            if (!W->fixed[i])
                for (int k = 0; k < 7; ++k) t += Ji[m * 7 + k] * W->p[7 * i + k];
            if (!W->fixed[j])
                for (int k = 0; k < 7; ++k) t += Jj[m * 7 + k] * W->p[7 * j + k];
            W->w[7 * (size_t)e + m] = t;
        }
    }
    for (int v = 0; v < W->n; ++v) {
        if (W->fixed[v]) continue;
        double acc[7];
        for (int k = 0; k < 7; ++k) acc[k] = 0.0;
        for (int s = W->adj_off[v]; s < W->adj_off[v + 1]; ++s) {
            const int e = W->adj[s] >> 1;
            const double *J = ((W->adj[s] & 1) ? W->Jj : W->Ji) + 49 * (size_t)e, *w = W->w + 7 * (size_t)e;
            for (int k = 0; k < 7; ++k) {
                double t = 0.0;
                for (int m = 0; m < 7; ++m) t += J[m * 7 + k] * w[m];
                acc[k] += t;
            }
        }
        for (int k = 0; k < 7; ++k) W->q[7 * v + k] = acc[k] + lambda * W->p[7 * v + k];
        if (W->fix_scale) W->q[7 * v + 6] = W->p[7 * v + 6];
    }
}

/* preconditioned CG from x = 0; returns the iterations run, *capped = 1 when the cap ended it */
static int pg_cg(const pg_work *W, double lambda, double tol, int cap, int *capped)
{
    const int n = W->n;
    for (int v = 0; v < n; ++v) {
        if (W->fixed[v]) continue;
        for (int k = 0; k < 7; ++k) { W->x[7 * v + k] = 0.0; W->r[7 * v + k] = W->b[7 * v + k]; }
        pg_chol7_solve(W->Lf + 28 * v, W->r + 7 * v, W->z + 7 * v);
        for (int k = 0; k < 7; ++k) W->p[7 * v + k] = W->z[7 * v + k];
    }
    double rz = pg_dot(W->r, W->z, W->fixed, n);
    const double stop = (tol * tol) * rz;
    int it = 0;
    *capped = 0;
    for (;;) {
        if (rz <= stop) break;
        if (it >= cap) { *capped = 1; break; }
        pg_apply(W, lambda);
        const double pq = pg_dot(W->p, W->q, W->fixed, n);
        if (!(pq > 0)) break;
        const double alpha = rz / pq;
        for (int v = 0; v < n; ++v) {
            if (W->fixed[v]) continue;
            for (int k = 0; k < 7; ++k) {
                W->x[7 * v + k] = W->x[7 * v + k] + alpha * W->p[7 * v + k];
                W->r[7 * v + k] = W->r[7 * v + k] - alpha * W->q[7 * v + k];
            }
            pg_chol7_solve(W->Lf + 28 * v, W->r + 7 * v, W->z + 7 * v);
        }
        const double rzn = pg_dot(W->r, W->z, W->fixed, n);
        const double beta = rzn / rz;
        for (int v = 0; v < n; ++v) {
            if (W->fixed[v]) continue;
            for (int k = 0; k < 7; ++k) W->p[7 * v + k] = W->z[7 * v + k] + beta * W->p[7 * v + k];
        }
        rz = rzn;
        ++it;
    }
    return it;
}

/* the whole call; S_out receives the result (the input when status is PG_FAILED) */
void pg_optimize(int n, const double *S0, const uint8_t *fixed, int ne, const int32_t *edges, const double *M, const pg_params *prm,
                 double *S_out, pg_result *out)
{
    pg_work W;
    memset(&W, 0, sizeof W);
    memset(out, 0, sizeof *out);
    const size_t N = (size_t)n, E = (size_t)ne;
    int32_t *adj_off = (int32_t *)malloc(sizeof(int32_t) * (N + 1)), *adj = (int32_t *)malloc(sizeof(int32_t) * 2 * E);
    pg_adjacency(n, ne, edges, adj_off, adj);
    double *S = (double *)malloc(sizeof(double) * 8 * N), *Sn = (double *)malloc(sizeof(double) * 8 * N);
    W.n = n; W.ne = ne; W.fix_scale = prm->fix_scale != 0; W.fixed = fixed; W.edges = edges; W.adj_off = adj_off; W.adj = adj;
    W.Ji = (double *)calloc(49 * E, sizeof(double)); W.Jj = (double *)calloc(49 * E, sizeof(double));
    W.res = (double *)calloc(7 * E, sizeof(double)); W.w = (double *)calloc(7 * E, sizeof(double));
    W.D = (double *)calloc(28 * N, sizeof(double)); W.Lf = (double *)calloc(28 * N, sizeof(double));
    W.b = (double *)calloc(7 * N, sizeof(double)); W.x = (double *)calloc(7 * N, sizeof(double));
    W.r = (double *)calloc(7 * N, sizeof(double)); W.z = (double *)calloc(7 * N, sizeof(double));
    W.p = (double *)calloc(7 * N, sizeof(double)); W.q = (double *)calloc(7 * N, sizeof(double));
    memcpy(S, S0, sizeof(double) * 8 * N);
    int n_free = 0;
    for (int v = 0; v < n; ++v) n_free += !fixed[v];
    int cap = prm->cg_max_iterations;
    if (cap <= 0) cap = 7 * n_free < PG_CG_CAP ? 7 * n_free : PG_CG_CAP;

    double lambda = 0.0, ni = 2.0, currentChi = 0.0;
    int status = PG_MAX_ITERATIONS;
    for (int it = 0; it < prm->max_iterations; ++it) {
        double cost;
        const int lin_ok = pg_linearize(n, S, ne, edges, M, W.fix_scale, W.res, W.Ji, W.Jj, &cost);
        if (it == 0) {
            if (!lin_ok) { status = PG_FAILED; break; }
            out->cost_initial = cost;
        }
        currentChi = cost;                                           /* an accepted trial passed the same checks: lin_ok holds */
        pg_gather_system(&W);
        if (it == 0) {
            double mx = 0.0;
            for (int v = 0; v < n; ++v) {
                if (fixed[v]) continue;
                int m = 0;
                for (int a = 0; a < 7; ++a) { const double h = fabs(W.D[28 * v + m]); if (h > mx) mx = h; m += 7 - a; }
            }
            lambda = 1e-5 * mx; ni = 2.0;
        }
        double rho = 0.0;
        int qmax = 0, converged = 0;
        do {
            int ok = 1;
            for (int v = 0; v < n; ++v)
                if (!fixed[v]) ok &= pg_chol7(W.D + 28 * v, lambda, W.fix_scale, W.Lf + 28 * v);
            double tempChi = PG_DMAX;
            if (ok) {
                int capped = 0;
                out->cg_iterations_total += pg_cg(&W, lambda, prm->cg_tol, cap, &capped);
                out->cg_capped += capped;
                ++out->n_solves;
                for (int v = 0; v < n; ++v) {
                    int zero = 1;
                    if (!fixed[v])
                        for (int k = 0; k < 7; ++k) zero &= W.x[7 * v + k] == 0.0;
                    if (fixed[v] || zero) memcpy(Sn + 8 * v, S + 8 * v, sizeof(double) * 8);
                    else ok &= pg_retract(S + 8 * v, W.x + 7 * v, Sn + 8 * v);
                }
            }
            if (ok) {
                ok = pg_cost(Sn, ne, edges, M, &tempChi);
                if (!ok) tempChi = PG_DMAX;
            }
            rho = currentChi - tempChi;
            double scale = 0.0;
            if (ok) {
                double lane[PG_LANES];
                for (int l = 0; l < PG_LANES; ++l) {
                    double acc = 0.0;
                    for (int v = l; v < n; v += PG_LANES) {
                        if (fixed[v]) continue;
                        for (int k = 0; k < 7; ++k) acc += W.x[7 * v + k] * (lambda * W.x[7 * v + k] + W.b[7 * v + k]);
                    }
                    lane[l] = acc;
                }
                scale = pg_tree(lane);
            }
            scale += 1e-3;
            rho = rho / scale;
            if (ok && rho > 0 && fabs(tempChi) <= PG_DMAX) {
                const double u = 2.0 * rho - 1.0;
                double alpha = 1.0 - u * u * u;
                if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                lambda = lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
                ni = 2.0;
                converged = currentChi - tempChi <= prm->min_rel_decrease * currentChi;
                currentChi = tempChi;
                memcpy(S, Sn, sizeof(double) * 8 * N);
            } else {
                lambda = lambda * ni; ni = ni * 2.0;
                if (!(fabs(lambda) <= PG_DMAX)) break;
            }
            ++qmax;
        } while (rho < 0 && qmax < prm->max_trials);
        ++out->lm_iterations;
        if (qmax == prm->max_trials || rho == 0 || !(fabs(lambda) <= PG_DMAX)) { status = PG_STALLED; break; }
        if (converged) { status = PG_CONVERGED; break; }
    }
    out->status = status;
    out->cost_final = status == PG_FAILED ? 0.0 : currentChi;
    out->lambda = lambda;
    memcpy(S_out, status == PG_FAILED ? S0 : S, sizeof(double) * 8 * N);
    free(adj_off); free(adj); free(S); free(Sn);
    free(W.Ji); free(W.Jj); free(W.res); free(W.w); free(W.D); free(W.Lf); free(W.b); free(W.x); free(W.r); free(W.z); free(W.p); free(W.q);
}
