/* gba_ref.c -- restatement of the global bundle adjustment (ygz_slam_amd/csrc/gba.hip): the yardstick of tests/test_gba_ref.py and
 * tests/test_gpu_gba.py, and the frozen spec of DESIGN.md section 15.  What ORB-SLAM2's Optimizer::GlobalBundleAdjustemnt leaves to g2o and
 * Eigen is stated here function by function in the kernels' operation order.  Test infrastructure: plain C99, single-threaded, built by
 * tests/gba_ref.py with -O2 -ffp-contract=off -fno-fast-math, never linked into the product.  Only + - * / and sqrt.
 *
 *  - a pose is T (world -> camera) stored qx qy qz qw tx ty tz, a point X three numbers; an edge (pose, point, pixel) has the residual
 *    r = obs - K (R X + t) / z, identity information and g2o's Huber kernel of width huber_delta (<= 0: none);
 *  - Jacobians analytic at Delta = 0 in camera coordinates P = R X + t: dP/d(omega, t) = [-[P]x, I], dP/dX = R, chained through the pinhole;
 *  - retraction T <- Delta(d) o T with q_Delta = normalise(omega / 2, 1), t <- R_Delta t + dt; a point moves additively; a vertex whose step
 *    is exactly zero keeps its bits;
 *  - outer loop: Levenberg-Marquardt with g2o's rules (pgo_ref.c's) and a relative-decrease stop;
 *  - inner solve: the points are marginalised; preconditioned conjugate gradients on the reduced camera system S d = b~, S never assembled,
 *    the preconditioner the Cholesky factor of every free pose's 6x6 diagonal block of S;
 *  - sums: over a point's edges in edge-index order (a CSR list); over a pose's edges lane-strided over GB_LANES lanes in the order of its
 *    CSR list, then the tree 128 .. 1; over the poses lane-strided in index order, then the tree; over all edges or all points in two
 *    levels: chunks of GB_CHUNK consecutive elements, each lane-strided and tree-summed, then the chunk sums lane-strided in chunk order and
 *    tree-summed. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define GB_LANES 256           /* lanes of every workgroup of gba.hip */
#define GB_CHUNK 1024          /* elements per first-level chunk of a two-level sum: four per lane */
#define GB_CG_CAP 1024         /* bound of the automatic CG cap */
#define GB_DMAX 1.7976931348623157e308

enum { GB_FAILED = 0, GB_CONVERGED = 1, GB_MAX_ITERATIONS = 2, GB_STALLED = 3 };

/* the layouts of ygz_gba_params and ygz_gba_result (include/ygz_hip.h) */
typedef struct {
    int32_t max_iterations, max_trials, cg_max_iterations, cg_batch;
    double  cg_tol, min_rel_decrease;
} gb_params;

typedef struct {
    double  cost_initial, cost_final, lambda;
    int32_t status, lm_iterations, n_solves, cg_iterations_total, cg_capped, pad;
} gb_result;

typedef struct {
    int n, nl, ne;
    const double *poses, *points, *obs;      /* [N][7], [L][3], [E][2] */
    const uint8_t *fixed;
    const int32_t *edge_pose, *edge_point;
    double fx, fy, cx, cy, delta;
} gb_problem;

/* ---- one edge ------------------------------------------------------------------------------------------------------------------ */
/* on the device: ygz_quat_rotation (ygz_slam_amd/csrc/posemath_dev.h) */
void gb_rotation(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

/* P = R X + t, r = obs - (f P_xy / P_z + c); 0 when the depth is not positive or a value is not finite */
int gb_residual(const double *T, const double *X, const double *ob, const double *K, double *R, double *P, double *r)
{
    gb_rotation(T, R);
    for (int i = 0; i < 3; ++i) P[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2]) + T[4 + i];
    if (!(P[2] > 0)) return 0;
    const double xn = P[0] / P[2], yn = P[1] / P[2];
    r[0] = ob[0] - (K[0] * xn + K[2]);
    r[1] = ob[1] - (K[1] * yn + K[3]);
    return fabs(r[0]) <= GB_DMAX && fabs(r[1]) <= GB_DMAX;
}

/* g2o's RobustKernelHuber: rho and rho' at e2 = |r|^2 */
void gb_robust(const double *r, double delta, double *rho0, double *rho1)
{
    const double e2 = r[0] * r[0] + r[1] * r[1], dsqr = delta * delta;
    *rho0 = e2; *rho1 = 1.0;
    if (delta > 0 && e2 > dsqr) {
        const double s = sqrt(e2);
        *rho0 = 2.0 * s * delta - dsqr;
        *rho1 = delta / s;
    }
}

/* residual r [2], weight w, cost term rho, Jp = dr/d(omega, t) [2][6], Jl = dr/dX [2][3]; 0 (and zeros) when the residual is rejected */
int gb_edge_terms(const double *T, const double *X, const double *ob, const double *K, double delta, double *r, double *w, double *rho,
                  double *Jp, double *Jl)
{
    double R[9], P[3];
    if (!gb_residual(T, X, ob, K, R, P, r)) {
        r[0] = 0.0; r[1] = 0.0; *w = 0.0; *rho = 0.0;
        for (int k = 0; k < 12; ++k) Jp[k] = 0.0;
        for (int k = 0; k < 6; ++k) Jl[k] = 0.0;
        return 0;
    }
    gb_robust(r, delta, rho, w);
    const double x = P[0], y = P[1], z = P[2];
    const double iz = 1.0 / z, a = K[0] * iz, b = K[1] * iz, c = K[0] * (x / z) * iz, d = K[1] * (y / z) * iz;
    Jp[0] = c * y;         Jp[1] = -(a * z) - c * x; Jp[2] = a * y;    Jp[3] = -a;  Jp[4] = 0.0; Jp[5] = c;
    Jp[6] = b * z + d * y; Jp[7] = -(d * x);         Jp[8] = -(b * x); Jp[9] = 0.0; Jp[10] = -b; Jp[11] = d;
    for (int k = 0; k < 3; ++k) {
        Jl[k] = -(a * R[k]) + c * R[6 + k];
        Jl[3 + k] = -(b * R[3 + k]) + d * R[6 + k];
    }
    return 1;
}

/* Hpl = w Jp^T Jl, 6x3 row-major */
void gb_hpl(const double *Jp, const double *Jl, double w, double *H)
{
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 3; ++b) H[3 * a + b] = w * (Jp[a] * Jl[b] + Jp[6 + a] * Jl[3 + b]);
}

/* T <- Delta(d) o T, d = (omega, t) */
/* on the device: ygz_se3_retract (ygz_slam_amd/csrc/posemath_dev.h) */
void gb_retract(const double *T, const double *d, double *out)
{
    double dq[4] = { 0.5 * d[0], 0.5 * d[1], 0.5 * d[2], 1.0 };
    const double dn = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    for (int k = 0; k < 4; ++k) dq[k] = dq[k] / dn;
    const double ax = dq[0], ay = dq[1], az = dq[2], aw = dq[3], bx = T[0], by = T[1], bz = T[2], bw = T[3];
    double q[4];
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by - ax * bz + ay * bw + az * bx;
    q[2] = aw * bz + ax * by - ay * bx + az * bw;
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
    double dR[9];
    gb_rotation(dq, dR);
    for (int i = 0; i < 3; ++i) out[4 + i] = (dR[3 * i] * T[4] + dR[3 * i + 1] * T[5] + dR[3 * i + 2] * T[6]) + d[3 + i];
}

/* ---- small dense blocks ---------------------------------------------------------------------------------------------------------- */
/* the inverse of the symmetric 3x3 A + lambda I through its LDL^T; A and inv are upper triangles (00 01 02 11 12 22); 0 on a non-positive
 * pivot */
int gb_inv3(const double *A, double lambda, double *inv)
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

/* o = M v for the symmetric 3x3 M given as an upper triangle */
static void gb_sym3_mul(const double *M, const double *v, double *o)
{
    o[0] = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
    o[1] = M[1] * v[0] + M[3] * v[1] + M[4] * v[2];
    o[2] = M[2] * v[0] + M[4] * v[1] + M[5] * v[2];
}

/* D: the upper triangle row by row (21); Lo: the Cholesky factor, lower triangle row by row (21); 0 on a non-positive pivot */
/* on the device: ygz_sym_unpack and ygz_chol_factor (ygz_slam_amd/csrc/posemath_dev.h) */
int gb_chol6(const double *D, double *Lo)
{
    double A[36], L[36];
    int m = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { A[a * 6 + b] = D[m]; A[b * 6 + a] = D[m]; ++m; }
    for (int k = 0; k < 36; ++k) L[k] = 0.0;
    int ok = 1;
    for (int j = 0; j < 6; ++j) {
        double d = A[j * 6 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
        ok &= d > 0;
        const double ljj = sqrt(d);
        L[j * 6 + j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i * 6 + j];
            for (int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k];
            L[i * 6 + j] = v / ljj;
        }
    }
    m = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) Lo[m++] = L[i * 6 + j];
    return ok;
}

/* x = (L L^T)^-1 b */
/* on the device: ygz_chol_solve_packed (ygz_slam_amd/csrc/posemath_dev.h) */
void gb_chol6_solve(const double *Lo, const double *b, double *x)
{
    double L[36], y[6];
    int m = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) L[i * 6 + j] = Lo[m++];
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
}

/* ---- sums ------------------------------------------------------------------------------------------------------------------------ */
static double gb_tree(double *lane)
{
    for (int st = GB_LANES / 2; st >= 1; st /= 2)
        for (int l = 0; l < st; ++l) lane[l] += lane[l + st];
    return lane[0];
}

/* one level: lane-strided in index order, then the tree */
static double gb_sum1(const double *v, int n)
{
    double lane[GB_LANES];
    for (int l = 0; l < GB_LANES; ++l) {
        double acc = 0.0;
        for (int i = l; i < n; i += GB_LANES) acc += v[i];
        lane[l] = acc;
    }
    return gb_tree(lane);
}

/* two levels: chunks of GB_CHUNK elements by gb_sum1, the chunk sums by gb_sum1 */
double gb_sum2(const double *v, int n)
{
    const int nc = (n + GB_CHUNK - 1) / GB_CHUNK;
    double *part = (double *)malloc(sizeof(double) * (size_t)(nc > 0 ? nc : 1));
    for (int c = 0; c < nc; ++c) {
        const int m = n - c * GB_CHUNK < GB_CHUNK ? n - c * GB_CHUNK : GB_CHUNK;
        part[c] = gb_sum1(v + (size_t)c * GB_CHUNK, m);
    }
    const double s = gb_sum1(part, nc);
    free(part);
    return s;
}

/* the CSR list of `key` [E] over n_keys keys: off [n_keys + 1], adj [E] the edges of each key in edge-index order */
void gb_csr(int n_keys, int ne, const int32_t *key, int32_t *off, int32_t *adj)
{
    for (int v = 0; v <= n_keys; ++v) off[v] = 0;
    for (int e = 0; e < ne; ++e) ++off[key[e] + 1];
    for (int v = 0; v < n_keys; ++v) off[v + 1] += off[v];
    int32_t *fill = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n_keys > 0 ? n_keys : 1));
    for (int v = 0; v < n_keys; ++v) fill[v] = off[v];
    for (int e = 0; e < ne; ++e) adj[fill[key[e]]++] = e;
    free(fill);
}

/* ---- the work ---------------------------------------------------------------------------------------------------------------------- */
typedef struct {
    gb_problem pb;
    double K[4];
    int32_t *pt_off, *pt_adj, *ps_off, *ps_adj;
    double *T, *X, *Tn, *Xn;                              /* the estimate and the trial */
    double *res, *w, *Jp, *Jl, *Hpl, *term;               /* [E][2], [E], [E][12], [E][6], [E][18], [E] */
    double *Hpp, *bp, *Hll, *bl;                          /* [N][21], [N][6], [L][6], [L][3] */
    double *Hinv, *wl, *vl, *dl, *lterm;                  /* [L][6], [L][3], [L][3], [L][3], [L] */
    double *bt, *Lf, *x, *r, *z, *p, *q, *vterm;          /* [N][6], [N][21], 5 x [N][6], [N] */
} gb_work;

/* residuals, weights, Jacobian blocks, Hpl and the cost at (T, X); 0 when an edge is rejected */
static int gb_linearize_edges(gb_work *W, const double *T, const double *X, double *cost)
{
    const gb_problem *pb = &W->pb;
    int ok = 1;
    for (int e = 0; e < pb->ne; ++e) {
        ok &= gb_edge_terms(T + 7 * pb->edge_pose[e], X + 3 * pb->edge_point[e], pb->obs + 2 * (size_t)e, W->K, pb->delta, W->res + 2 * (size_t)e,
                            W->w + e, W->term + e, W->Jp + 12 * (size_t)e, W->Jl + 6 * (size_t)e);
        gb_hpl(W->Jp + 12 * (size_t)e, W->Jl + 6 * (size_t)e, W->w[e], W->Hpl + 18 * (size_t)e);
    }
    *cost = gb_sum2(W->term, pb->ne);
    return ok && fabs(*cost) <= GB_DMAX;
}

/* the cost alone at (T, X) */
static int gb_cost(gb_work *W, const double *T, const double *X, double *cost)
{
    const gb_problem *pb = &W->pb;
    int ok = 1;
    for (int e = 0; e < pb->ne; ++e) {
        double R[9], P[3], r[2], w;
        W->term[e] = 0.0;
        if (!gb_residual(T + 7 * pb->edge_pose[e], X + 3 * pb->edge_point[e], pb->obs + 2 * (size_t)e, W->K, R, P, r)) { ok = 0; continue; }
        gb_robust(r, pb->delta, W->term + e, &w);
    }
    *cost = gb_sum2(W->term, pb->ne);
    return ok && fabs(*cost) <= GB_DMAX;
}

/* Hll, bl per point (edge-index order) and Hpp, bp per free pose (lane-strided over its list, then the tree) */
static void gb_gather_system(gb_work *W)
{
    const gb_problem *pb = &W->pb;
    for (int l = 0; l < pb->nl; ++l) {
        double h[6], g[3];
        for (int k = 0; k < 6; ++k) h[k] = 0.0;
        for (int k = 0; k < 3; ++k) g[k] = 0.0;
        for (int s = W->pt_off[l]; s < W->pt_off[l + 1]; ++s) {
            const int e = W->pt_adj[s];
            const double *J = W->Jl + 6 * (size_t)e, *r = W->res + 2 * (size_t)e, w = W->w[e];
            int m = 0;
            for (int a = 0; a < 3; ++a) {
                for (int b = a; b < 3; ++b) h[m++] += w * (J[a] * J[b] + J[3 + a] * J[3 + b]);
                g[a] += w * (J[a] * r[0] + J[3 + a] * r[1]);
            }
        }
        for (int k = 0; k < 6; ++k) W->Hll[6 * (size_t)l + k] = h[k];
        for (int k = 0; k < 3; ++k) W->bl[3 * (size_t)l + k] = -g[k];
    }
    for (int v = 0; v < pb->n; ++v) {
        if (pb->fixed[v]) continue;
        double lane[27][GB_LANES];
        for (int ln = 0; ln < GB_LANES; ++ln) {
            double acc[27];
            for (int k = 0; k < 27; ++k) acc[k] = 0.0;
            for (int s = W->ps_off[v] + ln; s < W->ps_off[v + 1]; s += GB_LANES) {
                const int e = W->ps_adj[s];
                const double *J = W->Jp + 12 * (size_t)e, *r = W->res + 2 * (size_t)e, w = W->w[e];
                int m = 0;
                for (int a = 0; a < 6; ++a) {
                    for (int b = a; b < 6; ++b) acc[m++] += w * (J[a] * J[b] + J[6 + a] * J[6 + b]);
                    acc[21 + a] += w * (J[a] * r[0] + J[6 + a] * r[1]);
                }
            }
            for (int k = 0; k < 27; ++k) lane[k][ln] = acc[k];
        }
        for (int k = 0; k < 21; ++k) W->Hpp[21 * v + k] = gb_tree(lane[k]);
        for (int k = 0; k < 6; ++k) W->bp[6 * v + k] = -gb_tree(lane[21 + k]);
    }
}

/* per point: Hinv = (Hll + lambda I)^-1 and wl = Hinv bl; per free pose: bt = bp - sum Hpl wl and the factor of
 * Hpp + lambda I - sum Hpl Hinv Hpl^T; 0 on a non-positive pivot */
static int gb_trial_system(gb_work *W, double lambda)
{
    const gb_problem *pb = &W->pb;
    int ok = 1;
    for (int l = 0; l < pb->nl; ++l) {
        ok &= gb_inv3(W->Hll + 6 * (size_t)l, lambda, W->Hinv + 6 * (size_t)l);
        gb_sym3_mul(W->Hinv + 6 * (size_t)l, W->bl + 3 * (size_t)l, W->wl + 3 * (size_t)l);
    }
    for (int v = 0; v < pb->n; ++v) {
        if (pb->fixed[v]) continue;
        double lane[27][GB_LANES];
        for (int ln = 0; ln < GB_LANES; ++ln) {
            double acc[27];
            for (int k = 0; k < 27; ++k) acc[k] = 0.0;
            for (int s = W->ps_off[v] + ln; s < W->ps_off[v + 1]; s += GB_LANES) {
                const int e = W->ps_adj[s], l = pb->edge_point[e];
                const double *H = W->Hpl + 18 * (size_t)e, *Hi = W->Hinv + 6 * (size_t)l, *wl = W->wl + 3 * (size_t)l;
                double Tm[18];
                for (int a = 0; a < 6; ++a) {
                    gb_sym3_mul(Hi, H + 3 * a, Tm + 3 * a);                       /* row a of Hpl Hinv (Hinv is symmetric) */
                    acc[21 + a] += H[3 * a] * wl[0] + H[3 * a + 1] * wl[1] + H[3 * a + 2] * wl[2];
                }
                int m = 0;
                for (int a = 0; a < 6; ++a)
                    for (int b = a; b < 6; ++b) acc[m++] += Tm[3 * a] * H[3 * b] + Tm[3 * a + 1] * H[3 * b + 1] + Tm[3 * a + 2] * H[3 * b + 2];
            }
            for (int k = 0; k < 27; ++k) lane[k][ln] = acc[k];
        }
        double D[21];
        int m = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) {
                const double h = a == b ? W->Hpp[21 * v + m] + lambda : W->Hpp[21 * v + m];
                D[m] = h - gb_tree(lane[m]);
                ++m;
            }
        for (int k = 0; k < 6; ++k) W->bt[6 * v + k] = W->bp[6 * v + k] - gb_tree(lane[21 + k]);
        ok &= gb_chol6(D, W->Lf + 21 * v);
    }
    return ok;
}

/* per point: out_l = sum over its edges with a free pose of Hpl^T y_pose, edge-index order */
static void gb_point_gather(const gb_work *W, const double *y, int l, double *u)
{
    const gb_problem *pb = &W->pb;
    u[0] = 0.0; u[1] = 0.0; u[2] = 0.0;
    for (int s = W->pt_off[l]; s < W->pt_off[l + 1]; ++s) {
        const int e = W->pt_adj[s], j = pb->edge_pose[e];
        if (pb->fixed[j]) continue;
        const double *H = W->Hpl + 18 * (size_t)e, *yj = y + 6 * j;
        for (int c = 0; c < 3; ++c) {
            double t = 0.0;
            for (int a = 0; a < 6; ++a) t += H[3 * a + c] * yj[a];
            u[c] += t;
        }
    }
}

/* q = S p over the free poses, and vterm_v = p_v . q_v */
static void gb_apply(gb_work *W, double lambda)
{
    const gb_problem *pb = &W->pb;
    for (int l = 0; l < pb->nl; ++l) {
        double u[3];
        gb_point_gather(W, W->p, l, u);
        gb_sym3_mul(W->Hinv + 6 * (size_t)l, u, W->vl + 3 * (size_t)l);
    }
    for (int v = 0; v < pb->n; ++v) {
        W->vterm[v] = 0.0;
        if (pb->fixed[v]) continue;
        double lane[6][GB_LANES];
        for (int ln = 0; ln < GB_LANES; ++ln) {
            double acc[6];
            for (int k = 0; k < 6; ++k) acc[k] = 0.0;
            for (int s = W->ps_off[v] + ln; s < W->ps_off[v + 1]; s += GB_LANES) {
                const int e = W->ps_adj[s];
                const double *H = W->Hpl + 18 * (size_t)e, *vl = W->vl + 3 * (size_t)pb->edge_point[e];
                for (int a = 0; a < 6; ++a) acc[a] += H[3 * a] * vl[0] + H[3 * a + 1] * vl[1] + H[3 * a + 2] * vl[2];
            }
            for (int k = 0; k < 6; ++k) lane[k][ln] = acc[k];
        }
        double A[36], d = 0.0;
        int m = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) { A[a * 6 + b] = W->Hpp[21 * v + m]; A[b * 6 + a] = W->Hpp[21 * v + m]; ++m; }
        const double *p = W->p + 6 * v;
        for (int a = 0; a < 6; ++a) {
            double t = 0.0;
            for (int b = 0; b < 6; ++b) t += A[a * 6 + b] * p[b];
            const double qa = (t + lambda * p[a]) - gb_tree(lane[a]);
            W->q[6 * v + a] = qa;
            d += p[a] * qa;
        }
        W->vterm[v] = d;
    }
}

/* sum over the free poses of a_v . b_v (fixed poses add 0) */
static double gb_dot(gb_work *W, const double *a, const double *b)
{
    const gb_problem *pb = &W->pb;
    for (int v = 0; v < pb->n; ++v) {
        double d = 0.0;
        if (!pb->fixed[v])
            for (int k = 0; k < 6; ++k) d += a[6 * v + k] * b[6 * v + k];
        W->vterm[v] = d;
    }
    return gb_sum1(W->vterm, pb->n);
}

/* preconditioned CG from x = 0 on S x = bt; returns the iterations run, *capped = 1 when the cap ended it */
static int gb_cg(gb_work *W, double lambda, double tol, int cap, int *capped)
{
    const gb_problem *pb = &W->pb;
    const int n = pb->n;
    for (int v = 0; v < n; ++v) {
        if (pb->fixed[v]) continue;
        for (int k = 0; k < 6; ++k) { W->x[6 * v + k] = 0.0; W->r[6 * v + k] = W->bt[6 * v + k]; }
        gb_chol6_solve(W->Lf + 21 * v, W->r + 6 * v, W->z + 6 * v);
        for (int k = 0; k < 6; ++k) W->p[6 * v + k] = W->z[6 * v + k];
    }
    double rz = gb_dot(W, W->r, W->z);
    const double stop = (tol * tol) * rz;
    int it = 0;
    *capped = 0;
    for (;;) {
        if (rz <= stop) break;
        if (it >= cap) { *capped = 1; break; }
        gb_apply(W, lambda);
        const double pq = gb_sum1(W->vterm, n);
        if (!(pq > 0)) break;
        const double alpha = rz / pq;
        for (int v = 0; v < n; ++v) {
            if (pb->fixed[v]) continue;
            for (int k = 0; k < 6; ++k) {
                W->x[6 * v + k] = W->x[6 * v + k] + alpha * W->p[6 * v + k];
                W->r[6 * v + k] = W->r[6 * v + k] - alpha * W->q[6 * v + k];
            }
            gb_chol6_solve(W->Lf + 21 * v, W->r + 6 * v, W->z + 6 * v);
        }
        const double rzn = gb_dot(W, W->r, W->z);
        const double beta = rzn / rz;
        for (int v = 0; v < n; ++v) {
            if (pb->fixed[v]) continue;
            for (int k = 0; k < 6; ++k) W->p[6 * v + k] = W->z[6 * v + k] + beta * W->p[6 * v + k];
        }
        rz = rzn;
        ++it;
    }
    return it;
}

/* the trial state (Tn, Xn) from x, and the denominator of rho without its 1e-3 */
static double gb_update(gb_work *W, double lambda)
{
    const gb_problem *pb = &W->pb;
    for (int l = 0; l < pb->nl; ++l) {
        double s[3], t[3], *dl = W->dl + 3 * (size_t)l;
        const double *bl = W->bl + 3 * (size_t)l, *X = W->X + 3 * (size_t)l;
        gb_point_gather(W, W->x, l, s);
        for (int c = 0; c < 3; ++c) t[c] = bl[c] - s[c];
        gb_sym3_mul(W->Hinv + 6 * (size_t)l, t, dl);
        const int zero = dl[0] == 0.0 && dl[1] == 0.0 && dl[2] == 0.0;
        double acc = 0.0;
        for (int c = 0; c < 3; ++c) {
            W->Xn[3 * (size_t)l + c] = zero ? X[c] : X[c] + dl[c];
            acc += dl[c] * (lambda * dl[c] + bl[c]);
        }
        W->lterm[l] = acc;
    }
    for (int v = 0; v < pb->n; ++v) {
        int zero = 1;
        double acc = 0.0;
        if (!pb->fixed[v])
            for (int k = 0; k < 6; ++k) {
                const double xk = W->x[6 * v + k];
                zero &= xk == 0.0;
                acc += xk * (lambda * xk + W->bp[6 * v + k]);
            }
        if (pb->fixed[v] || zero) memcpy(W->Tn + 7 * v, W->T + 7 * v, sizeof(double) * 7);
        else gb_retract(W->T + 7 * v, W->x + 6 * v, W->Tn + 7 * v);
        W->vterm[v] = acc;
    }
    return gb_sum1(W->vterm, pb->n) + gb_sum2(W->lterm, pb->nl);
}

static void gb_work_init(gb_work *W, const gb_problem *pb)
{
    memset(W, 0, sizeof *W);
    W->pb = *pb;
    W->K[0] = pb->fx; W->K[1] = pb->fy; W->K[2] = pb->cx; W->K[3] = pb->cy;
    const size_t N = (size_t)pb->n, L = (size_t)pb->nl, E = (size_t)pb->ne;
    W->pt_off = (int32_t *)malloc(sizeof(int32_t) * (L + 1)); W->pt_adj = (int32_t *)malloc(sizeof(int32_t) * E);
    W->ps_off = (int32_t *)malloc(sizeof(int32_t) * (N + 1)); W->ps_adj = (int32_t *)malloc(sizeof(int32_t) * E);
    gb_csr(pb->nl, pb->ne, pb->edge_point, W->pt_off, W->pt_adj);
    gb_csr(pb->n, pb->ne, pb->edge_pose, W->ps_off, W->ps_adj);
    W->T = (double *)malloc(sizeof(double) * 7 * N); W->Tn = (double *)malloc(sizeof(double) * 7 * N);
    W->X = (double *)malloc(sizeof(double) * 3 * L); W->Xn = (double *)malloc(sizeof(double) * 3 * L);
    memcpy(W->T, pb->poses, sizeof(double) * 7 * N);
    memcpy(W->X, pb->points, sizeof(double) * 3 * L);
    W->res = (double *)calloc(2 * E, sizeof(double)); W->w = (double *)calloc(E, sizeof(double)); W->Jp = (double *)calloc(12 * E, sizeof(double));
    W->Jl = (double *)calloc(6 * E, sizeof(double)); W->Hpl = (double *)calloc(18 * E, sizeof(double)); W->term = (double *)calloc(E, sizeof(double));
    W->Hpp = (double *)calloc(21 * N, sizeof(double)); W->bp = (double *)calloc(6 * N, sizeof(double));
    W->Hll = (double *)calloc(6 * L, sizeof(double)); W->bl = (double *)calloc(3 * L, sizeof(double));
    W->Hinv = (double *)calloc(6 * L, sizeof(double)); W->wl = (double *)calloc(3 * L, sizeof(double)); W->vl = (double *)calloc(3 * L, sizeof(double));
    W->dl = (double *)calloc(3 * L, sizeof(double)); W->lterm = (double *)calloc(L, sizeof(double));
    W->bt = (double *)calloc(6 * N, sizeof(double)); W->Lf = (double *)calloc(21 * N, sizeof(double)); W->x = (double *)calloc(6 * N, sizeof(double));
    W->r = (double *)calloc(6 * N, sizeof(double)); W->z = (double *)calloc(6 * N, sizeof(double)); W->p = (double *)calloc(6 * N, sizeof(double));
    W->q = (double *)calloc(6 * N, sizeof(double)); W->vterm = (double *)calloc(N, sizeof(double));
}

static void gb_work_free(gb_work *W)
{
    free(W->pt_off); free(W->pt_adj); free(W->ps_off); free(W->ps_adj); free(W->T); free(W->Tn); free(W->X); free(W->Xn);
    free(W->res); free(W->w); free(W->Jp); free(W->Jl); free(W->Hpl); free(W->term); free(W->Hpp); free(W->bp); free(W->Hll); free(W->bl);
    free(W->Hinv); free(W->wl); free(W->vl); free(W->dl); free(W->lterm); free(W->bt); free(W->Lf); free(W->x); free(W->r); free(W->z);
    free(W->p); free(W->q); free(W->vterm);
}

/* the stage: the linearisation at the input.  res [E][2], w [E], Jp [E][12], Jl [E][6], Hpp [N][21], bp [N][6], Hll [L][6], bl [L][3] (rows
 * of fixed poses are zero); each may be NULL.  Returns 1 when every residual is defined */
int gb_linearize(const gb_problem *pb, double *res, double *w, double *Jp, double *Jl, double *Hpp, double *bp, double *Hll, double *bl,
                 double *cost)
{
    gb_work W;
    gb_work_init(&W, pb);
    const size_t N = (size_t)pb->n, L = (size_t)pb->nl, E = (size_t)pb->ne;
    const int ok = gb_linearize_edges(&W, W.T, W.X, cost);
    gb_gather_system(&W);
    if (res) memcpy(res, W.res, sizeof(double) * 2 * E);
    if (w) memcpy(w, W.w, sizeof(double) * E);
    if (Jp) memcpy(Jp, W.Jp, sizeof(double) * 12 * E);
    if (Jl) memcpy(Jl, W.Jl, sizeof(double) * 6 * E);
    if (Hpp) memcpy(Hpp, W.Hpp, sizeof(double) * 21 * N);
    if (bp) memcpy(bp, W.bp, sizeof(double) * 6 * N);
    if (Hll) memcpy(Hll, W.Hll, sizeof(double) * 6 * L);
    if (bl) memcpy(bl, W.bl, sizeof(double) * 3 * L);
    gb_work_free(&W);
    return ok;
}

/* the whole call; poses_out / points_out receive the result (the input when status is GB_FAILED) */
void gb_optimize(const gb_problem *pb, const gb_params *prm, double *poses_out, double *points_out, gb_result *out)
{
    gb_work W;
    gb_work_init(&W, pb);
    memset(out, 0, sizeof *out);
    const size_t N = (size_t)pb->n, L = (size_t)pb->nl;
    int n_free = 0;
    for (int v = 0; v < pb->n; ++v) n_free += !pb->fixed[v];
    int cap = prm->cg_max_iterations;
    if (cap <= 0) cap = 6 * n_free < GB_CG_CAP ? 6 * n_free : GB_CG_CAP;

    double lambda = 0.0, ni = 2.0, currentChi = 0.0;
    int status = GB_MAX_ITERATIONS;
    for (int it = 0; it < prm->max_iterations; ++it) {
        double cost;
        const int lin_ok = gb_linearize_edges(&W, W.T, W.X, &cost);
        if (it == 0) {
            if (!lin_ok) { status = GB_FAILED; break; }
            out->cost_initial = cost;
        }
        currentChi = cost;                                           /* an accepted trial passed the same checks: lin_ok holds */
        gb_gather_system(&W);
        if (it == 0) {
            double mx = 0.0;
            for (int v = 0; v < pb->n; ++v) {
                if (pb->fixed[v]) continue;
                int m = 0;
                for (int a = 0; a < 6; ++a) { const double h = fabs(W.Hpp[21 * v + m]); if (h > mx) mx = h; m += 6 - a; }
            }
            for (int l = 0; l < pb->nl; ++l) {
                const int dg[3] = { 0, 3, 5 };
                for (int a = 0; a < 3; ++a) { const double h = fabs(W.Hll[6 * (size_t)l + dg[a]]); if (h > mx) mx = h; }
            }
            lambda = 1e-5 * mx; ni = 2.0;
        }
        double rho = 0.0;
        int qmax = 0, converged = 0;
        do {
            int ok = gb_trial_system(&W, lambda);
            double tempChi = GB_DMAX, scale = 0.0;
            if (ok) {
                int capped = 0;
                out->cg_iterations_total += gb_cg(&W, lambda, prm->cg_tol, cap, &capped);
                out->cg_capped += capped;
                ++out->n_solves;
                scale = gb_update(&W, lambda);
                ok = gb_cost(&W, W.Tn, W.Xn, &tempChi);
                if (!ok) { tempChi = GB_DMAX; scale = 0.0; }
            }
            scale += 1e-3;
            rho = (currentChi - tempChi) / scale;
            if (!(fabs(rho) <= GB_DMAX)) rho = -1.0;                 /* a step without a finite gain ratio is a rejected one */
            if (ok && rho > 0) {
                const double u = 2.0 * rho - 1.0;
                double alpha = 1.0 - u * u * u;
                if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                lambda = lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
                ni = 2.0;
                converged = currentChi - tempChi <= prm->min_rel_decrease * currentChi;
                currentChi = tempChi;
                memcpy(W.T, W.Tn, sizeof(double) * 7 * N);
                memcpy(W.X, W.Xn, sizeof(double) * 3 * L);
            } else {
                lambda = lambda * ni; ni = ni * 2.0;
                if (!(fabs(lambda) <= GB_DMAX)) break;
            }
            ++qmax;
        } while (rho < 0 && qmax < prm->max_trials);
        ++out->lm_iterations;
        if (qmax == prm->max_trials || rho == 0 || !(fabs(lambda) <= GB_DMAX)) { status = GB_STALLED; break; }
        if (converged) { status = GB_CONVERGED; break; }
    }
    out->status = status;
    out->cost_final = status == GB_FAILED ? 0.0 : currentChi;
    out->lambda = lambda;
    memcpy(poses_out, status == GB_FAILED ? pb->poses : W.T, sizeof(double) * 7 * N);
    memcpy(points_out, status == GB_FAILED ? pb->points : W.X, sizeof(double) * 3 * L);
    gb_work_free(&W);
}
