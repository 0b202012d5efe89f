/* pnp_ref.c -- restatement of the relocalisation pose solver (ygz_slam_amd/csrc/pnp.hip): the yardstick of tests/test_pnp_ref.py and
 * tests/test_gpu_pnp.py.  Nothing in the reference solves PnP (VisualOdometry.cpp:101-104 is a bare "try relocalization" comment), so
 * this file states the algorithm itself, function by function in the kernels' operation order.  Test
 * infrastructure: plain C99, single-threaded, built by tests/pnp_ref.py with -O2 -ffp-contract=off -fno-fast-math, never linked into
 * the product.
 *
 *  - sample sets: Initializer.cpp:33-49's scheme with 3 indices per iteration -- a fresh cv::RNG (state 0xffffffff) per problem,
 *    uniform(0, available) and the swap-remove of availableIndices;
 *  - minimal solver: Lambda Twist P3P (Persson & Nordberg, ECCV 2018) with only + - * / and sqrt: the cubic's largest real root by a
 *    bracket and 64 bisections, the two eigenvectors of the degenerate conic in closed form, 5 Gauss-Newton steps on the depths;
 *  - scoring: inlier = z > 0 and squared level-0 reprojection error <= chi2; score = inlier count;
 *  - selection: highest count, ties to the smallest hypothesis index (sample * 4 + solution); no hypothesis above 0: no winner. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define PR_MAX_SOL 4
#define PR_BISECT 64
#define PR_REFINE 5

/* the result block; the layout of ygz_pnp_result (include/ygz_hip.h) */
typedef struct {
    double  R[9], t[3], T_cw[7];
    int32_t success, n_inliers, best_sample, best_solution, n_hypotheses;
} pr_result;

/* ---- cv::RNG (OpenCV core/operations.hpp: RNG::next, RNG::uniform(int,int); default state 0xffffffff) --------------------- */
static uint32_t rng_next(uint64_t *s)
{
    *s = (uint64_t)(uint32_t)*s * 4164903690u + (uint32_t)(*s >> 32);
    return (uint32_t)*s;
}

/* the 3 distinct indices of every iteration (Initializer.cpp:33-49 with 3 in place of 8) */
void pr_sample_sets(int n, int max_iter, int32_t *sets)
{
    uint64_t st = 0xffffffffu;
    int32_t avail[n > 0 ? n : 1];
    for (int it = 0; it < max_iter; ++it) {
        int na = n;
        for (int i = 0; i < n; ++i) avail[i] = i;
        for (int j = 0; j < 3; ++j) {
            const int r = (int)(rng_next(&st) % (uint32_t)na);
            sets[it * 3 + j] = avail[r];
            avail[r] = avail[na - 1];
            --na;
        }
    }
}

/* ---- Lambda Twist ---------------------------------------------------------------------------------------------------------- */
/* real roots of x^2 + b x + c (the cancellation-free pair); 0 when there are none */
static int root2real(double b, double c, double *r1, double *r2)
{
    const double v = b * b - 4.0 * c;
    if (!(v >= 0)) { *r1 = 0; *r2 = 0; return 0; }
    const double y = sqrt(v);
    if (b < 0) { *r1 = 0.5 * (-b + y); *r2 = 2.0 * c / (-b + y); }
    else if (b > 0) { *r1 = 2.0 * c / (-b - y); *r2 = 0.5 * (-b - y); }
    else { *r1 = 0.5 * y; *r2 = -0.5 * y; }
    return 1;
}

static double cubic_at(double x, double b, double c, double d) { return ((x + b) * x + c) * x + d; }

/* the largest real root of x^3 + b x^2 + c x + d: a bracket on which the cubic is monotone, then PR_BISECT halvings */
double pr_cubic_root(double b, double c, double d)
{
    double B = fabs(b);
    if (fabs(c) > B) B = fabs(c);
    if (fabs(d) > B) B = fabs(d);
    B = B + 1.0;                                                /* Cauchy: every root lies in (-B, B) */
    double lo = -B, hi = B;
    const double disc = b * b - 3.0 * c;
    if (disc > 0) {
        const double sq = sqrt(disc);
        const double x1 = (-b - sq) / 3.0, x2 = (-b + sq) / 3.0;   /* local maximum, local minimum */
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

/* the eigenvectors of the two non-zero eigenvalues of the symmetric A (one eigenvalue is 0), larger |eigenvalue| first:
 * V[0..2] = v1, V[3..5] = v2, L = (e1, e2) */
void pr_eig_known0(const double *A, double *V, double *L)
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
    for (int k = 0; k < 2; ++k) {
        const double e = k == 0 ? e1 : e2;
        const double tmp = 1.0 / (e * e - e * (A[0] + A[4]) + mx2);     /* rows 0 and 1 of (A - e I) (a1, a2, 1)^T = 0 by Cramer */
        const double a1 = (e * A[2] + mx0) * tmp;
        const double a2 = (e * A[5] + mx1) * tmp;
        const double rn = 1.0 / sqrt(a1 * a1 + a2 * a2 + 1.0);
        V[3 * k + 0] = a1 * rn; V[3 * k + 1] = a2 * rn; V[3 * k + 2] = rn;
    }
}

static double residual_l1(const double *l, double a12, double a13, double a23, double b12, double b13, double b23, double *r)
{
    r[0] = l[0] * l[0] + l[1] * l[1] + b12 * l[0] * l[1] - a12;
    r[1] = l[0] * l[0] + l[2] * l[2] + b13 * l[0] * l[2] - a13;
    r[2] = l[1] * l[1] + l[2] * l[2] + b23 * l[1] * l[2] - a23;
    return fabs(r[0]) + fabs(r[1]) + fabs(r[2]);
}

/* PR_REFINE Gauss-Newton steps on the three depths; a step is taken only when it lowers the L1 residual */
void pr_refine(double *l, double a12, double a13, double a23, double b12, double b13, double b23)
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

static void bearing(const double *px, const double *K4, double *y)
{
    const double x = (px[0] - K4[2]) / K4[0], v = (px[1] - K4[3]) / K4[1];
    const double n = sqrt(x * x + v * v + 1.0);
    y[0] = x / n; y[1] = v / n; y[2] = 1.0 / n;
}

/* on the device: ygz_inv3 (ygz_slam_amd/csrc/posemath_dev.h) */
static void inv3(const double *a, double *r)
{
    double C[9];
    C[0] = a[4] * a[8] - a[5] * a[7]; C[1] = a[5] * a[6] - a[3] * a[8]; C[2] = a[3] * a[7] - a[4] * a[6];
    C[3] = a[2] * a[7] - a[1] * a[8]; C[4] = a[0] * a[8] - a[2] * a[6]; C[5] = a[1] * a[6] - a[0] * a[7];
    C[6] = a[1] * a[5] - a[2] * a[4]; C[7] = a[2] * a[3] - a[0] * a[5]; C[8] = a[0] * a[4] - a[1] * a[3];
    const double inv = 1.0 / (a[0] * C[0] + a[1] * C[1] + a[2] * C[2]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[i * 3 + j] = C[j * 3 + i] * inv;
}

/* R = Y X^-1, t = ry1 - R x1 for the depths l; 0 when a value is not finite */
static int pose_from_depths(const double *l, const double *y1, const double *y2, const double *y3, const double *x1, const double *Xi,
                            double *out)
{
    double r1[3], yd1[3], yd2[3], Y[9];
    for (int k = 0; k < 3; ++k) {
        r1[k] = y1[k] * l[0];
        yd1[k] = r1[k] - y2[k] * l[1];
        yd2[k] = r1[k] - y3[k] * l[2];
    }
    for (int k = 0; k < 3; ++k) { Y[k * 3 + 0] = yd1[k]; Y[k * 3 + 1] = yd2[k]; }
    Y[2] = yd1[1] * yd2[2] - yd1[2] * yd2[1];
    Y[5] = yd1[2] * yd2[0] - yd1[0] * yd2[2];
    Y[8] = yd1[0] * yd2[1] - yd1[1] * yd2[0];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[i * 3 + j] = Y[i * 3 + 0] * Xi[0 * 3 + j] + Y[i * 3 + 1] * Xi[1 * 3 + j] + Y[i * 3 + 2] * Xi[2 * 3 + j];
    for (int i = 0; i < 3; ++i) out[9 + i] = r1[i] - (out[i * 3 + 0] * x1[0] + out[i * 3 + 1] * x1[1] + out[i * 3 + 2] * x1[2]);
    int ok = 1;
    for (int k = 0; k < 12; ++k) ok &= fabs(out[k]) <= 1e300;     /* false for NaN and inf */
    return ok;
}

/* the P3P of three world points pw [3][3] and their level-0 pixels px [3][2]: up to 4 poses [4][12] (R row-major, t), camera = R pw + t;
 * the slots past the returned count are 0.  Candidate order: s = +v then -v, tau1 then tau2 (the compaction keeps it). */
int pr_p3p(const double *pw, const double *px, const double *K4, double *sol)
{
    for (int k = 0; k < 4 * 12; ++k) sol[k] = 0;
    const double *x1 = pw, *x2 = pw + 3, *x3 = pw + 6;
    double d12[3], d13[3], d23[3], nx[3];
    for (int k = 0; k < 3; ++k) { d12[k] = x1[k] - x2[k]; d13[k] = x1[k] - x3[k]; d23[k] = x2[k] - x3[k]; }
    nx[0] = d12[1] * d13[2] - d12[2] * d13[1];
    nx[1] = d12[2] * d13[0] - d12[0] * d13[2];
    nx[2] = d12[0] * d13[1] - d12[1] * d13[0];
    const double a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double a23 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
    const double nn = nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2];
    if (!(nn > 1e-10 * a12 * a13)) return 0;                    /* collinear or coincident world points */
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
    for (int k = 0; k < 3; ++k) { X[k * 3 + 0] = d12[k]; X[k * 3 + 1] = d13[k]; X[k * 3 + 2] = nx[k]; }
    inv3(X, Xi);
    int cnt = 0;
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
            for (int k = 0; k < 12; ++k) sol[cnt * 12 + k] = P[k];
            ++cnt;
        }
    }
    return cnt;
}

/* ---- scoring and selection --------------------------------------------------------------------------------------------------- */
static int pr_is_inlier(const double *P, const double *pw, const double *px, const double *K4, double chi2)
{
    const double X = P[0] * pw[0] + P[1] * pw[1] + P[2] * pw[2] + P[9];
    const double Y = P[3] * pw[0] + P[4] * pw[1] + P[5] * pw[2] + P[10];
    const double Z = P[6] * pw[0] + P[7] * pw[1] + P[8] * pw[2] + P[11];
    if (!(Z > 0)) return 0;
    const double du = K4[0] * (X / Z) + K4[2] - px[0];
    const double dv = K4[1] * (Y / Z) + K4[3] - px[1];
    return du * du + dv * dv <= chi2;
}

int pr_count(const double *P, const double *pw, const double *px, int n, const double *K4, double chi2, uint8_t *mask)
{
    int c = 0;
    for (int i = 0; i < n; ++i) {
        const int in = pr_is_inlier(P, pw + 3 * i, px + 2 * i, K4, chi2);
        if (mask) mask[i] = (uint8_t)in;
        c += in;
    }
    return c;
}

/* every hypothesis of one problem: solutions [max_iter][4][12], n_solutions [max_iter], counts [max_iter][4] (0 past n_solutions) */
void pr_hypotheses(const double *pw, const double *px, int n, const double *K4, const int32_t *sets, int max_iter, double chi2,
                   double *solutions, int32_t *n_solutions, int32_t *counts)
{
    for (int it = 0; it < max_iter; ++it) {
        double w[9], p[6];
        for (int j = 0; j < 3; ++j) {
            const int i = sets[it * 3 + j];
            w[3 * j] = pw[3 * i]; w[3 * j + 1] = pw[3 * i + 1]; w[3 * j + 2] = pw[3 * i + 2];
            p[2 * j] = px[2 * i]; p[2 * j + 1] = px[2 * i + 1];
        }
        double *sol = solutions + (size_t)it * 48;
        const int ns = pr_p3p(w, p, K4, sol);
        n_solutions[it] = ns;
        for (int k = 0; k < 4; ++k) counts[it * 4 + k] = k < ns ? pr_count(sol + 12 * k, pw, px, n, K4, chi2, NULL) : 0;
    }
}

/* Sophus SO3(const Matrix3d &) = Eigen::Quaterniond(const Matrix3d &): the trace branch, else the largest diagonal (qx qy qz qw) */
/* on the device: ygz_quat_from_matrix (ygz_slam_amd/csrc/posemath_dev.h) */
void pr_quat_from_matrix(const double *m, double *q)
{
    const double tr = m[0] + m[4] + m[8];
    if (tr > 0) {
        double t = sqrt(tr + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2 * 3 + 1] - m[1 * 3 + 2]) * t;
        q[1] = (m[0 * 3 + 2] - m[2 * 3 + 0]) * t;
        q[2] = (m[1 * 3 + 0] - m[0 * 3 + 1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 3 + i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double t = sqrt(m[i * 3 + i] - m[j * 3 + j] - m[k * 3 + k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
}

/* the winner among the hypotheses (highest count, ties to the smallest sample * 4 + solution; none when every count is 0), its pose,
 * T_cw and inlier mask [n] */
void pr_select(const double *pw, const double *px, int n, const double *K4, int max_iter, double chi2, int min_inliers,
               const double *solutions, const int32_t *n_solutions, const int32_t *counts, pr_result *r, uint8_t *inliers)
{
    memset(r, 0, sizeof *r);
    int best = -1, bc = 0, nh = 0;
    for (int h = 0; h < 4 * max_iter; ++h) {
        if (h % 4 < n_solutions[h / 4]) ++nh;
        if (counts[h] > bc) { bc = counts[h]; best = h; }
    }
    r->n_hypotheses = nh;
    r->R[0] = r->R[4] = r->R[8] = 1.0;
    r->T_cw[3] = 1.0;
    r->best_sample = -1; r->best_solution = -1;
    if (best < 0) {
        memset(inliers, 0, (size_t)n);
        return;
    }
    const double *P = solutions + (size_t)best * 12;
    for (int k = 0; k < 9; ++k) r->R[k] = P[k];
    for (int k = 0; k < 3; ++k) r->t[k] = P[9 + k];
    pr_quat_from_matrix(r->R, r->T_cw);
    for (int k = 0; k < 3; ++k) r->T_cw[4 + k] = r->t[k];
    r->best_sample = best / 4; r->best_solution = best % 4;
    r->n_inliers = pr_count(P, pw, px, n, K4, chi2, inliers);
    r->success = r->n_inliers >= min_inliers;
}

/* the whole call for one problem: the sets of (n, max_iter), every hypothesis, the selection.  Work arrays from the caller:
 * solutions [max_iter * 48], n_solutions [max_iter], counts [max_iter * 4], sets [max_iter * 3]. */
void pr_ransac(const double *pw, const double *px, int n, const double *K4, int max_iter, double chi2, int min_inliers, int32_t *sets,
               double *solutions, int32_t *n_solutions, int32_t *counts, pr_result *r, uint8_t *inliers)
{
    pr_sample_sets(n, max_iter, sets);
    pr_hypotheses(pw, px, n, K4, sets, max_iter, chi2, solutions, n_solutions, counts);
    pr_select(pw, px, n, K4, max_iter, chi2, min_inliers, solutions, n_solutions, counts, r, inliers);
}
