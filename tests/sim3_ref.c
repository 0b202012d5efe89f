/* sim3_ref.c -- restatement of the loop detection's Sim3 solver (ygz_slam_amd/csrc/sim3.hip): the yardstick of tests/test_sim3_ref.py and
 * tests/test_gpu_sim3.py.  Nothing in the reference solves Sim3 (LocalMapping.cpp:330 ends in a comment, loop_closing.h is an empty class),
 * so this file states the algorithm itself, function by function in the kernels' operation order.  Test
 * infrastructure: plain C99, single-threaded, built by tests/sim3_ref.py with -O2 -ffp-contract=off -fno-fast-math, never linked into the
 * product.  Only + - * / and sqrt.
 *
 *  - sample sets: those of pnp_ref.c (cv::RNG, 3 indices per iteration);
 *  - minimal solver: Horn 1987 on 3 correspondences, as ORB-SLAM2's Sim3Solver::ComputeSim3 -- centroids, M = sum Pr2 Pr1^T, the 4x4 N,
 *    its largest eigenvector by cyclic Jacobi with a fixed schedule, the scale of Horn's asymmetric form, t12 = O1 - s R12 O2;
 *  - scoring (Sim3Solver::CheckInliers): both projections in front and within chi2 * 4^level of the observed pixel;
 *  - selection: highest count, ties to the smallest sample; no count above 0: no winner;
 *  - refinement (Optimizer::OptimizeSim3): LM of g2o's rules on the 7-dof S12, two Huber-weighted reprojection edges per pair; the FP64
 *    sums over pairs are lane-strided over SR_LANES lanes in pair order, then a fixed tree over the lanes (the kernel's block). */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define SR_SWEEPS 8            /* Jacobi sweeps over the 6 pairs */
#define SR_LANES 256           /* lanes of k_sim3_refine */
#define SR_NSUM 36             /* H (28, upper triangle row by row), b (7), chi (1) */
#define SR_DMAX 1.7976931348623157e308

/* the result block; the layout of ygz_sim3_result (include/ygz_hip.h) */
typedef struct {
    double  S12[8], S21[8];
    double  chi2_ransac, chi2_refined;
    int32_t success, n_hypotheses, best_sample, n_inliers, n_refined, lm_iterations;
} sr_result;

typedef struct {
    int    max_iter;
    double chi2;
    int    min_inliers;
    double chi2_refine;
    int    iters_first, iters_more, iters_again, fix_scale;
} sr_params;

/* ---- cv::RNG sample sets (pnp_ref.c's) --------------------------------------------------------------------------------------- */
static uint32_t rng_next(uint64_t *s)
{
    *s = (uint64_t)(uint32_t)*s * 4164903690u + (uint32_t)(*s >> 32);
    return (uint32_t)*s;
}

void sr_sample_sets(int n, int max_iter, int32_t *sets)
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

/* ---- Sim3 algebra: S = (q, t, s) stored as qx qy qz qw tx ty tz s; S X = s (R X) + t ----------------------------------------- */
/* on the device: ygz_quat_rotation (ygz_slam_amd/csrc/posemath_dev.h) */
void sr_rotation(const double *q, double *R)
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

/* S (8) -> R (9), the acting form */
static void sim3_act(const double *S, const double *R, const double *X, double *P)
{
    double r[3];
    mat_vec(R, X, r);
    for (int k = 0; k < 3; ++k) P[k] = S[7] * r[k] + S[4 + k];
}

/* S21 = S12^-1: (1/s, R^T (the conjugate quaternion), -(1/s) R^T t) */
/* on the device: ygz_sim3_inverse (ygz_slam_amd/csrc/posemath_dev.h) */
void sr_inverse(const double *S, double *Si)
{
    Si[0] = -S[0]; Si[1] = -S[1]; Si[2] = -S[2]; Si[3] = S[3];
    Si[7] = 1.0 / S[7];
    double R[9], r[3];
    sr_rotation(Si, R);
    mat_vec(R, S + 4, r);
    for (int k = 0; k < 3; ++k) Si[4 + k] = -(Si[7] * r[k]);
}

/* ---- Horn's closed form ----------------------------------------------------------------------------------------------------- */
/* cyclic Jacobi on the symmetric 4x4 A (destroyed): V's columns are the eigenvectors, A's diagonal the eigenvalues */
void sr_jacobi4(double *A, double *V)
{
    static const int PP[6] = { 0, 0, 0, 1, 1, 2 }, QQ[6] = { 1, 2, 3, 2, 3, 3 };
    for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sw = 0; sw < SR_SWEEPS; ++sw)
        for (int pr = 0; pr < 6; ++pr) {
            const int p = PP[pr], q = QQ[pr];
            const double apq = A[p * 4 + q];
            if (apq == 0.0) continue;
            const double theta = (A[q * 4 + q] - A[p * 4 + p]) / (2.0 * apq);
            double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
            if (theta < 0) t = -t;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            A[p * 4 + p] = A[p * 4 + p] - t * apq;
            A[q * 4 + q] = A[q * 4 + q] + t * apq;
            A[p * 4 + q] = 0.0; A[q * 4 + p] = 0.0;
            for (int r = 0; r < 4; ++r) {
                if (r == p || r == q) continue;
                const double arp = A[r * 4 + p], arq = A[r * 4 + q];
                const double np = c * arp - s * arq, nq = s * arp + c * arq;
                A[r * 4 + p] = np; A[p * 4 + r] = np;
                A[r * 4 + q] = nq; A[q * 4 + r] = nq;
            }
            for (int r = 0; r < 4; ++r) {
                const double vrp = V[r * 4 + p], vrq = V[r * 4 + q];
                V[r * 4 + p] = c * vrp - s * vrq;
                V[r * 4 + q] = s * vrp + c * vrq;
            }
        }
}

/* S12 (and S21) with S12 X2 ~ X1 from n correspondences X1 [n][3], X2 [n][3]; 0 when s <= 0 or a value is not finite */
int sr_horn(const double *X1, const double *X2, int n, int fix_scale, double *S12, double *S21)
{
    double O1[3] = { 0, 0, 0 }, O2[3] = { 0, 0, 0 };
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) { O1[k] += X1[3 * i + k]; O2[k] += X2[3 * i + k]; }
    for (int k = 0; k < 3; ++k) { O1[k] = O1[k] / n; O2[k] = O2[k] / n; }
    double M[9];
    for (int k = 0; k < 9; ++k) M[k] = 0.0;
    for (int i = 0; i < n; ++i) {
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) { a[k] = X2[3 * i + k] - O2[k]; b[k] = X1[3 * i + k] - O1[k]; }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) M[3 * r + c] += a[r] * b[c];          /* M = sum Pr2 Pr1^T */
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
    int best = 0;
    for (int i = 1; i < 4; ++i) if (N[i * 5] > N[best * 5]) best = i;
    double w = V[0 * 4 + best], x = V[1 * 4 + best], y = V[2 * 4 + best], z = V[3 * 4 + best];
    const double nq = sqrt(w * w + x * x + y * y + z * z);
    w = w / nq; x = x / nq; y = y / nq; z = z / nq;
    if (w < 0) { w = -w; x = -x; y = -y; z = -z; }
    S12[0] = x; S12[1] = y; S12[2] = z; S12[3] = w;
    double R[9];
    sr_rotation(S12, R);
    double s = 1.0;
    if (!fix_scale) {
        double num = 0.0, den = 0.0;
        for (int i = 0; i < n; ++i) {
            double a[3], b[3], r[3];
            for (int k = 0; k < 3; ++k) { a[k] = X2[3 * i + k] - O2[k]; b[k] = X1[3 * i + k] - O1[k]; }
            mat_vec(R, a, r);
            num += b[0] * r[0] + b[1] * r[1] + b[2] * r[2];
            den += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        }
        s = num / den;
    }
    S12[7] = s;
    double ro[3];
    mat_vec(R, O2, ro);
    for (int k = 0; k < 3; ++k) S12[4 + k] = O1[k] - s * ro[k];
    sr_inverse(S12, S21);
    int ok = s > 0;
    for (int k = 0; k < 8; ++k) ok &= fabs(S12[k]) <= SR_DMAX && fabs(S21[k]) <= SR_DMAX;
    return ok;
}

static int sr_collinear(const double *X)
{
    double d12[3], d13[3], nx[3];
    for (int k = 0; k < 3; ++k) { d12[k] = X[k] - X[3 + k]; d13[k] = X[k] - X[6 + k]; }
    nx[0] = d12[1] * d13[2] - d12[2] * d13[1];
    nx[1] = d12[2] * d13[0] - d12[0] * d13[2];
    nx[2] = d12[0] * d13[1] - d12[1] * d13[0];
    const double a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double nn = nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2];
    return !(nn > 1e-10 * a12 * a13);
}

/* one sample: X1, X2 [3][3] -> hyp [16] = S12 (8), S21 (8); 0 (and identities) when invalid */
int sr_solve3(const double *X1, const double *X2, int fix_scale, double *hyp)
{
    int ok = !sr_collinear(X1) && !sr_collinear(X2);
    if (ok) ok = sr_horn(X1, X2, 3, fix_scale, hyp, hyp + 8);
    if (!ok)
        for (int k = 0; k < 16; ++k) hyp[k] = (k % 8 == 3 || k % 8 == 7) ? 1.0 : 0.0;
    return ok;
}

/* ---- scoring --------------------------------------------------------------------------------------------------------------- */
double sr_sigma2(int level)
{
    double s2 = 1.0;
    for (int k = 0; k < level; ++k) s2 = s2 * 4.0;
    return s2;
}

/* the squared level-0 reprojection error of P against u; 0 into *front when P is not in front */
static double reproj2(const double *P, const double *u, const double *K4, int *front)
{
    *front = P[2] > 0;
    const double du = K4[0] * (P[0] / P[2]) + K4[2] - u[0];
    const double dv = K4[1] * (P[1] / P[2]) + K4[3] - u[1];
    return du * du + dv * dv;
}

/* S (8) and its R (9) for both directions */
static int sr_is_inlier(const double *S12, const double *R12, const double *S21, const double *R21, const double *X1, const double *X2,
                        const double *u1, const double *u2, const double *K4, double th1, double th2)
{
    double P[3], Q[3];
    int f1, f2;
    sim3_act(S12, R12, X2, P);
    sim3_act(S21, R21, X1, Q);
    const double e1 = reproj2(P, u1, K4, &f1);
    const double e2 = reproj2(Q, u2, K4, &f2);
    return f1 && f2 && e1 < th1 && e2 < th2;
}

int sr_count(const double *hyp, const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels, int n,
             const double *K4, double chi2, uint8_t *mask)
{
    double R12[9], R21[9];
    sr_rotation(hyp, R12);
    sr_rotation(hyp + 8, R21);
    int c = 0;
    for (int i = 0; i < n; ++i) {
        const double th1 = chi2 * sr_sigma2(levels[2 * i]), th2 = chi2 * sr_sigma2(levels[2 * i + 1]);
        const int in = sr_is_inlier(hyp, R12, hyp + 8, R21, X1 + 3 * i, X2 + 3 * i, px1 + 2 * i, px2 + 2 * i, K4, th1, th2);
        if (mask) mask[i] = (uint8_t)in;
        c += in;
    }
    return c;
}

/* every sample of one problem: hyps [max_iter][16], valid [max_iter], counts [max_iter] (0 when invalid) */
void sr_hypotheses(const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels, int n, const double *K4,
                   const int32_t *sets, int max_iter, double chi2, int fix_scale, double *hyps, int32_t *valid, int32_t *counts)
{
    for (int it = 0; it < max_iter; ++it) {
        double a[9], b[9];
        for (int j = 0; j < 3; ++j) {
            const int i = sets[it * 3 + j];
            for (int k = 0; k < 3; ++k) { a[3 * j + k] = X1[3 * i + k]; b[3 * j + k] = X2[3 * i + k]; }
        }
        double *h = hyps + (size_t)it * 16;
        valid[it] = sr_solve3(a, b, fix_scale, h);
        counts[it] = valid[it] ? sr_count(h, X1, X2, px1, px2, levels, n, K4, chi2, NULL) : 0;
    }
}

/* ---- refinement ------------------------------------------------------------------------------------------------------------ */
/* the left-multiplicative update S <- Delta(x) o S, x = (omega, t, sigma); 0 when |sigma| >= 2 */
/* on the device: ygz_sim3_retract (ygz_slam_amd/csrc/posemath_dev.h) */
int sr_apply_delta(const double *S, const double *x, double *out)
{
    if (!(fabs(x[6]) < 2.0)) return 0;
    double dq[4] = { 0.5 * x[0], 0.5 * x[1], 0.5 * x[2], 1.0 };
    const double dn = sqrt(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]);
    for (int k = 0; k < 4; ++k) dq[k] = dq[k] / dn;
    const double ds = (2.0 + x[6]) / (2.0 - x[6]);
    /* q = dq * q (Hamilton, x y z w) */
    const double ax = dq[0], ay = dq[1], az = dq[2], aw = dq[3], bx = S[0], by = S[1], bz = S[2], bw = S[3];
    double q[4];
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by - ax * bz + ay * bw + az * bx;
    q[2] = aw * bz + ax * by - ay * bx + az * bw;
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
    const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
    double dR[9], r[3];
    sr_rotation(dq, dR);
    mat_vec(dR, S + 4, r);
    for (int k = 0; k < 3; ++k) out[4 + k] = ds * r[k] + x[3 + k];
    out[7] = ds * S[7];
    return 1;
}

/* the residual of one edge: e = u - pi(P), J = -dpi/dP D (D: dP/dx, 3 x 7) */
static void edge_jacobian(const double *P, const double *D, const double *K4, double *J)
{
    const double iz = 1.0 / P[2];
    const double a = K4[0] * iz, b = K4[1] * iz;
    const double c = -(K4[0] * P[0]) * (iz * iz), d = -(K4[1] * P[1]) * (iz * iz);
    for (int k = 0; k < 7; ++k) {
        J[k] = -(a * D[k] + c * D[14 + k]);
        J[7 + k] = -(b * D[7 + k] + d * D[14 + k]);
    }
}

/* the two edges of one pair at S12: residuals e12, e21 (2 each), Jacobians J12, J21 ([2][7] each), chi2 (e^T e / sigma^2) of both */
void sr_pair_terms(const double *S, const double *X1, const double *X2, const double *u1, const double *u2, int l1, int l2, const double *K4,
                   int fix_scale, double *e12, double *e21, double *J12, double *J21, double *c12, double *c21)
{
    double R[9], Si[8], Ri[9], P[3], Q[3], D[21];
    sr_rotation(S, R);
    sr_inverse(S, Si);
    sr_rotation(Si, Ri);
    sim3_act(S, R, X2, P);
    sim3_act(Si, Ri, X1, Q);
    e12[0] = u1[0] - (K4[0] * (P[0] / P[2]) + K4[2]);
    e12[1] = u1[1] - (K4[1] * (P[1] / P[2]) + K4[3]);
    e21[0] = u2[0] - (K4[0] * (Q[0] / Q[2]) + K4[2]);
    e21[1] = u2[1] - (K4[1] * (Q[1] / Q[2]) + K4[3]);
    /* dP/dx = [-[P]x, I, P] */
    const double G1[21] = { 0.0, P[2], -P[1], 1.0, 0.0, 0.0, P[0],
                            -P[2], 0.0, P[0], 0.0, 1.0, 0.0, P[1],
                            P[1], -P[0], 0.0, 0.0, 0.0, 1.0, P[2] };
    for (int k = 0; k < 21; ++k) D[k] = G1[k];
    if (fix_scale) D[6] = D[13] = D[20] = 0.0;
    edge_jacobian(P, D, K4, J12);
    /* dQ/dx = (1/s) R^T [[X1]x, -I, -X1] */
    const double G2[21] = { 0.0, -X1[2], X1[1], -1.0, 0.0, 0.0, -X1[0],
                            X1[2], 0.0, -X1[0], 0.0, -1.0, 0.0, -X1[1],
                            -X1[1], X1[0], 0.0, 0.0, 0.0, -1.0, -X1[2] };
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 7; ++k) D[7 * r + k] = Si[7] * (Ri[3 * r] * G2[k] + Ri[3 * r + 1] * G2[7 + k] + Ri[3 * r + 2] * G2[14 + k]);
    if (fix_scale) D[6] = D[13] = D[20] = 0.0;
    edge_jacobian(Q, D, K4, J21);
    const double i1 = 1.0 / sr_sigma2(l1), i2 = 1.0 / sr_sigma2(l2);
    *c12 = (e12[0] * e12[0] + e12[1] * e12[1]) * i1;
    *c21 = (e21[0] * e21[0] + e21[1] * e21[1]) * i2;
}

/* g2o's Huber: rho(c) and the weight rho'(c) */
static double huber(double c, double delta, double d2, double *w)
{
    if (c <= d2) { *w = 1.0; return c; }
    const double sq = sqrt(c);
    *w = delta / sq;
    return 2.0 * delta * sq - d2;
}

static void add_edge(double *acc, const double *J, const double *e, double c, double info, double delta, double d2)
{
    double w;
    const double rho = huber(c, delta, d2, &w);
    const double wi = w * info;
    int m = 0;
    for (int a = 0; a < 7; ++a)
        for (int b = a; b < 7; ++b) acc[m++] += wi * (J[a] * J[b] + J[7 + a] * J[7 + b]);
    for (int a = 0; a < 7; ++a) acc[28 + a] -= wi * (J[a] * e[0] + J[7 + a] * e[1]);
    acc[35] += rho;
}

/* sum over the active pairs (act[i] & bit) of H, b and chi (with_h) or of chi alone: lane-strided partial sums, then the tree */
static void sr_accumulate(const double *S, const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels,
                          int n, const double *K4, int fix_scale, double chi2_refine, const uint8_t *act, int bit, int with_h, double *tot)
{
    static double lane[SR_LANES][SR_NSUM];
    const double delta = sqrt(chi2_refine), d2 = chi2_refine;
    memset(lane, 0, sizeof lane);
    for (int l = 0; l < SR_LANES; ++l)
        for (int i = l; i < n; i += SR_LANES) {
            if (!(act[i] & bit)) continue;
            double e12[2], e21[2], J12[14], J21[14], c12, c21;
            sr_pair_terms(S, X1 + 3 * i, X2 + 3 * i, px1 + 2 * i, px2 + 2 * i, levels[2 * i], levels[2 * i + 1], K4, fix_scale, e12, e21, J12,
                          J21, &c12, &c21);
            if (with_h) {
                add_edge(lane[l], J12, e12, c12, 1.0 / sr_sigma2(levels[2 * i]), delta, d2);
                add_edge(lane[l], J21, e21, c21, 1.0 / sr_sigma2(levels[2 * i + 1]), delta, d2);
            } else {
                double w;
                lane[l][35] += huber(c12, delta, d2, &w);
                lane[l][35] += huber(c21, delta, d2, &w);
            }
        }
    for (int st = SR_LANES / 2; st >= 1; st /= 2)
        for (int l = 0; l < st; ++l)
            for (int k = 0; k < SR_NSUM; ++k) lane[l][k] += lane[l + st][k];
    for (int k = 0; k < SR_NSUM; ++k) tot[k] = lane[0][k];
}

/* (H + lambda I) x = b by Cholesky; with fix_scale the scale row / column is the identity; 0 on a non-positive pivot */
int sr_solve7(const double *tot, double lambda, int fix_scale, double *x)
{
    double A[49], L[49], y[7];
    int m = 0;
    for (int a = 0; a < 7; ++a)
        for (int b = a; b < 7; ++b) { A[a * 7 + b] = tot[m]; A[b * 7 + a] = tot[m]; ++m; }
    for (int a = 0; a < 7; ++a) A[a * 7 + a] = A[a * 7 + a] + lambda;
    double bb[7];
    for (int a = 0; a < 7; ++a) bb[a] = tot[28 + a];
    if (fix_scale) {
        for (int a = 0; a < 7; ++a) { A[a * 7 + 6] = 0.0; A[6 * 7 + a] = 0.0; }
        A[48] = 1.0; bb[6] = 0.0;
    }
    for (int k = 0; k < 49; ++k) L[k] = 0.0;
    for (int j = 0; j < 7; ++j) {
        double d = A[j * 7 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 7 + k] * L[j * 7 + k];
        if (!(d > 0)) return 0;
        const double ljj = sqrt(d);
        L[j * 7 + j] = ljj;
        for (int i = j + 1; i < 7; ++i) {
            double v = A[i * 7 + j];
            for (int k = 0; k < j; ++k) v -= L[i * 7 + k] * L[j * 7 + k];
            L[i * 7 + j] = v / ljj;
        }
    }
    for (int i = 0; i < 7; ++i) {
        double v = bb[i];
        for (int k = 0; k < i; ++k) v -= L[i * 7 + k] * y[k];
        y[i] = v / L[i * 7 + i];
    }
    for (int i = 6; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 7; ++k) v -= L[k * 7 + i] * x[k];
        x[i] = v / L[i * 7 + i];
    }
    return 1;
}

/* one optimize(iters) call of g2o's LM (oracle/ceres_ba.c yo_g2o_lm's rules) on S over the pairs with act & bit; returns the final sum
 * of rho, the start's into *chi0; *its += iterations run */
static double sr_lm(double *S, const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels, int n,
                    const double *K4, int fix_scale, double chi2_refine, const uint8_t *act, int bit, int iters, double *chi0, int *its)
{
    double tot[SR_NSUM], tmp[SR_NSUM], Sb[8], x[7];
    double lambda = 0.0, ni = 2.0, currentChi = 0.0;
    for (int it = 0; it < iters; ++it) {
        sr_accumulate(S, X1, X2, px1, px2, levels, n, K4, fix_scale, chi2_refine, act, bit, 1, tot);
        currentChi = tot[35];
        if (it == 0) {
            *chi0 = currentChi;
            double mx = 0.0;
            int m = 0;
            for (int a = 0; a < 7; ++a) { const double h = fabs(tot[m]); if (h > mx) mx = h; m += 7 - a; }
            lambda = 1e-5 * mx; ni = 2.0;
        }
        double rho = 0.0;
        int qmax = 0;
        do {
            for (int k = 0; k < 8; ++k) Sb[k] = S[k];
            int ok = sr_solve7(tot, lambda, fix_scale, x);
            double tempChi = SR_DMAX;
            if (ok) ok = sr_apply_delta(Sb, x, S);
            if (ok) {
                sr_accumulate(S, X1, X2, px1, px2, levels, n, K4, fix_scale, chi2_refine, act, bit, 0, tmp);
                tempChi = tmp[35];
            }
            rho = currentChi - tempChi;
            double scale = 0.0;
            if (ok)
                for (int d = 0; d < 7; ++d) scale += x[d] * (lambda * x[d] + tot[28 + d]);
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
                for (int k = 0; k < 8; ++k) S[k] = Sb[k];
                if (!(fabs(lambda) <= SR_DMAX)) break;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);
        ++*its;
        if (qmax == 10 || rho == 0 || !(fabs(lambda) <= SR_DMAX)) break;
    }
    return currentChi;
}

/* Optimizer::OptimizeSim3's schedule on the RANSAC winner r (mask bit 0: its inliers); sets bit 1 of mask on the refined inliers */
void sr_refine(const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels, int n, const double *K4,
               const sr_params *p, sr_result *r, uint8_t *mask)
{
    double S[8];
    for (int k = 0; k < 8; ++k) S[k] = r->S12[k];
    int its = 0, drops = 0;
    double chi0 = 0.0, tmp = 0.0;
    sr_lm(S, X1, X2, px1, px2, levels, n, K4, p->fix_scale, p->chi2_refine, mask, 1, p->iters_first, &chi0, &its);
    for (int i = 0; i < n; ++i) {
        if (!(mask[i] & 1)) continue;
        double e12[2], e21[2], J12[14], J21[14], c12, c21;
        sr_pair_terms(S, X1 + 3 * i, X2 + 3 * i, px1 + 2 * i, px2 + 2 * i, levels[2 * i], levels[2 * i + 1], K4, p->fix_scale, e12, e21, J12, J21,
                      &c12, &c21);
        if (!(c12 <= p->chi2_refine && c21 <= p->chi2_refine)) ++drops;
        else mask[i] |= 2;
    }
    const double chi = sr_lm(S, X1, X2, px1, px2, levels, n, K4, p->fix_scale, p->chi2_refine, mask, 2, drops > 0 ? p->iters_more : p->iters_again,
                             &tmp, &its);
    int nin = 0;
    for (int i = 0; i < n; ++i) {
        if (!(mask[i] & 2)) continue;
        double e12[2], e21[2], J12[14], J21[14], c12, c21;
        sr_pair_terms(S, X1 + 3 * i, X2 + 3 * i, px1 + 2 * i, px2 + 2 * i, levels[2 * i], levels[2 * i + 1], K4, p->fix_scale, e12, e21, J12, J21,
                      &c12, &c21);
        if (!(c12 <= p->chi2_refine && c21 <= p->chi2_refine)) mask[i] &= (uint8_t)~2u;
        else ++nin;
    }
    for (int k = 0; k < 8; ++k) r->S12[k] = S[k];
    sr_inverse(S, r->S21);
    r->chi2_ransac = chi0;
    r->chi2_refined = chi;
    r->lm_iterations = its;
    r->n_refined = nin;
    r->success = nin >= p->min_inliers;
}

/* the winner among the samples (highest count, ties to the smallest; none when every count is 0), its mask (bit 0), then -- when RANSAC
 * succeeded -- the refinement */
void sr_select(const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels, int n, const double *K4,
               const sr_params *p, const double *hyps, const int32_t *valid, const int32_t *counts, sr_result *r, uint8_t *mask)
{
    memset(r, 0, sizeof *r);
    int best = -1, bc = 0, nh = 0;
    for (int h = 0; h < p->max_iter; ++h) {
        nh += valid[h] != 0;
        if (counts[h] > bc) { bc = counts[h]; best = h; }
    }
    r->n_hypotheses = nh;
    r->S12[3] = r->S12[7] = r->S21[3] = r->S21[7] = 1.0;
    r->best_sample = -1;
    if (best < 0) {
        memset(mask, 0, (size_t)n);
        return;
    }
    const double *h = hyps + (size_t)best * 16;
    for (int k = 0; k < 8; ++k) { r->S12[k] = h[k]; r->S21[k] = h[8 + k]; }
    r->best_sample = best;
    r->n_inliers = sr_count(h, X1, X2, px1, px2, levels, n, K4, p->chi2, mask);
    if (r->n_inliers >= p->min_inliers) sr_refine(X1, X2, px1, px2, levels, n, K4, p, r, mask);
}

/* the whole call for one problem.  Work arrays from the caller: sets [max_iter * 3], hyps [max_iter * 16], valid, counts [max_iter] */
void sr_ransac(const double *X1, const double *X2, const double *px1, const double *px2, const int32_t *levels, int n, const double *K4,
               const sr_params *p, int32_t *sets, double *hyps, int32_t *valid, int32_t *counts, sr_result *r, uint8_t *mask)
{
    sr_sample_sets(n, p->max_iter, sets);
    sr_hypotheses(X1, X2, px1, px2, levels, n, K4, sets, p->max_iter, p->chi2, p->fix_scale, hyps, valid, counts);
    sr_select(X1, X2, px1, px2, levels, n, K4, p, hyps, valid, counts, r, mask);
}
