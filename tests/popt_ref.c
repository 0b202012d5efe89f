/* popt_ref.c -- restatement of the stereo pose optimisation (ygz_slam_amd/csrc/popt.hip): the yardstick of tests/test_popt_ref.py and
 * tests/test_gpu_popt.py, and the frozen spec of DESIGN.md section 20.  What ORB-SLAM2's Optimizer::PoseOptimization leaves to g2o and Eigen is
 * stated here function by function in the kernel's operation order.  Test infrastructure: plain C99, single-threaded, built by tests/popt_ref.py
 * with -O2 -ffp-contract=off -fno-fast-math, never linked into the product.  Only + - * / and sqrt.
 *
 *  - a pose is T (world -> camera) stored qx qy qz qw tx ty tz; rotation matrix and retraction are gb_rotation and gb_retract of tests/gba_ref.c;
 *  - an edge has a world point X, an observation (u, v, uR), a pyramid level and a kind (0 absent, 1 mono, 2 stereo); its weight is
 *    w = 4^-level; r0 = u - (fx x/z + cx), r1 = v - (fy y/z + cy), stereo r2 = uR - (fx x/z + cx - bf/z); chi2 = w |r|^2; g2o's Huber kernel on
 *    chi2 with delta^2 = chi2_mono or chi2_stereo;
 *  - an edge is rejected in an evaluation when !(z > 0) or a residual is not finite: it adds nothing to any sum and is counted;
 *  - sums over a frame's active edges: lane l of PR_LANES takes the edges l, l + 256, ... in that order; the 256 lane sums are reduced per
 *    wavefront of 64 lanes (inside a row of 16 lanes the tree over adjacent pairs, then ((row0 + row1) + row2) + row3), then
 *    ((wave0 + wave1) + wave2) + wave3: pr_reduce;
 *  - every round restarts from the entry pose; Levenberg-Marquardt with g2o's rules as gb_optimize of tests/gba_ref.c states them, the solve a
 *    dense Cholesky of H + lambda I; a trial is failed on a bad pivot, on a non-finite cost, or when more edges are rejected at the trial pose
 *    than at the iteration's linearisation;
 *  - after the round every edge with kind != 0 is classified by a fresh evaluation at the round's pose. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define PR_LANES 256
#define PR_MAX_ROUNDS 8
#define PR_DMAX 1.7976931348623157e308

enum { PR_FAILED = 0, PR_CONVERGED = 1, PR_MAX_ITERATIONS = 2, PR_STALLED = 3 };
/* the codes of the trial trace: a trial that was evaluated and accepted, evaluated and rejected, failed after its pass (cost or rejected edges),
 * or failed at the pivot (no pass) */
enum { PR_TRIAL_ACCEPTED = 1, PR_TRIAL_REJECTED = 0, PR_TRIAL_FAILED = 2, PR_TRIAL_PIVOT = 3 };

/* the layout of ygz_pose_opt_params (include/ygz_hip.h) */
typedef struct {
    double  baseline, chi2_mono, chi2_stereo;
    int32_t rounds, iterations, max_trials, robust_rounds, min_edges, min_inliers;
    double  min_rel_decrease;
} pr_params;

int pr_params_size(void) { return (int)sizeof(pr_params); }

void pr_default_params(pr_params *p)
{
    p->baseline = 0.0; p->chi2_mono = 5.991; p->chi2_stereo = 7.815;
    p->rounds = 4; p->iterations = 10; p->max_trials = 10; p->robust_rounds = 3; p->min_edges = 3; p->min_inliers = 10;
    p->min_rel_decrease = 0.0;
}

/* ---- one edge -------------------------------------------------------------------------------------------------------------------- */
/* on the device: ygz_quat_rotation (ygz_slam_amd/csrc/posemath_dev.h) */
void pr_rotation(const double *q, double *R)
{
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

/* T <- Delta(d) o T, d = (omega, t) */
/* on the device: ygz_se3_retract (ygz_slam_amd/csrc/posemath_dev.h) */
void pr_retract(const double *T, const double *d, double *out)
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
    pr_rotation(dq, dR);
    for (int i = 0; i < 3; ++i) out[4 + i] = (dR[3 * i] * T[4] + dR[3 * i + 1] * T[5] + dR[3 * i + 2] * T[6]) + d[3 + i];
}

/* w = 4^-level */
/* on the device: ygz_level_weight (ygz_slam_amd/csrc/posemath_dev.h) */
static double pr_weight(int level) { return 1.0 / (double)(1 << (2 * level)); }

/* P = R X + t and the residuals r [3] (r[2] = 0 for a mono edge); K = fx fy cx cy bf; 0 when the edge is rejected */
int pr_residual(const double *R, const double *t, const double *X, const double *ob, int kind, const double *K, double *P, double *r)
{
    for (int i = 0; i < 3; ++i) P[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2]) + t[i];
    if (!(P[2] > 0)) return 0;
    const double xn = P[0] / P[2], yn = P[1] / P[2], up = K[0] * xn + K[2];
    r[0] = ob[0] - up;
    r[1] = ob[1] - (K[1] * yn + K[3]);
    r[2] = 0.0;
    if (kind == 2) r[2] = ob[2] - (up - K[4] / P[2]);
    return fabs(r[0]) <= PR_DMAX && fabs(r[1]) <= PR_DMAX && fabs(r[2]) <= PR_DMAX;
}

double pr_chi2(const double *r, int kind, double w)
{
    double e2 = r[0] * r[0] + r[1] * r[1];
    if (kind == 2) e2 = e2 + r[2] * r[2];
    return w * e2;
}

/* g2o's RobustKernelHuber on chi2: d2 = delta^2 (<= 0: no kernel), delta = sqrt(d2) */
void pr_robust(double chi2, double d2, double delta, double *rho0, double *rho1)
{
    *rho0 = chi2; *rho1 = 1.0;
    if (d2 > 0 && chi2 > d2) {
        const double s = sqrt(chi2);
        *rho0 = 2.0 * s * delta - d2;
        *rho1 = delta / s;
    }
}

/* the Jacobian rows dr/d(omega, t) at Delta = 0: J [3][6] (row 2 is zero for a mono edge) */
void pr_jacobian(const double *P, int kind, const double *K, double *J)
{
    const double x = P[0], y = P[1], z = P[2];
    const double iz = 1.0 / z, a = K[0] * iz, b = K[1] * iz, c = K[0] * (x / z) * iz, d = K[1] * (y / z) * iz;
    J[0] = c * y;         J[1] = -(a * z) - c * x; J[2] = a * y;    J[3] = -a;  J[4] = 0.0; J[5] = c;
    J[6] = b * z + d * y; J[7] = -(d * x);         J[8] = -(b * x); J[9] = 0.0; J[10] = -b; J[11] = d;
    for (int k = 0; k < 6; ++k) J[12 + k] = 0.0;
    if (kind == 2) {
        const double e = (K[4] * iz) * iz;
        J[12] = J[0] - e * y; J[13] = J[1] + e * x; J[14] = J[2]; J[15] = J[3]; J[16] = 0.0; J[17] = J[5] - e;
    }
}

/* one edge's share of a linearisation: acc [0..20] += rho' w J^T J (upper triangle), acc [21..26] += rho' w J^T r, acc [27] += rho; 0 when the
 * edge is rejected (nothing is added) */
int pr_edge_terms(const double *R, const double *t, const double *X, const double *ob, int level, int kind, const double *K, double d2,
                  double delta, double *acc)
{
    double P[3], r[3], J[18], rho0, rho1;
    if (!pr_residual(R, t, X, ob, kind, K, P, r)) return 0;
    const double w = pr_weight(level);
    pr_robust(pr_chi2(r, kind, w), d2, delta, &rho0, &rho1);
    pr_jacobian(P, kind, K, J);
    const double ww = rho1 * w;
    int m = 0;
    for (int a = 0; a < 6; ++a) {
        for (int b = a; b < 6; ++b) {
            double h = J[a] * J[b] + J[6 + a] * J[6 + b];
            if (kind == 2) h = h + J[12 + a] * J[12 + b];
            acc[m] += ww * h;
            ++m;
        }
        double g = J[a] * r[0] + J[6 + a] * r[1];
        if (kind == 2) g = g + J[12 + a] * r[2];
        acc[21 + a] += ww * g;
    }
    acc[27] += rho0;
    return 1;
}

/* one edge's share of a cost-only pass */
int pr_edge_cost(const double *R, const double *t, const double *X, const double *ob, int level, int kind, const double *K, double d2,
                 double delta, double *acc)
{
    double P[3], r[3], rho0, rho1;
    if (!pr_residual(R, t, X, ob, kind, K, P, r)) return 0;
    pr_robust(pr_chi2(r, kind, pr_weight(level)), d2, delta, &rho0, &rho1);
    acc[27] += rho0;
    return 1;
}

/* ---- sums -------------------------------------------------------------------------------------------------------------------------- */
/* the 256 lane sums: per wavefront of 64 the rows of 16 by the tree over adjacent pairs, ((r0 + r1) + r2) + r3, then the four wavefronts in
 * order */
double pr_reduce(const double *lane)
{
    double wave[4];
    for (int wv = 0; wv < 4; ++wv) {
        double row[4];
        for (int rw = 0; rw < 4; ++rw) {
            double v[16];
            for (int i = 0; i < 16; ++i) v[i] = lane[64 * wv + 16 * rw + i];
            for (int n = 8; n >= 1; n /= 2)
                for (int i = 0; i < n; ++i) v[i] = v[2 * i] + v[2 * i + 1];
            row[rw] = v[0];
        }
        wave[wv] = ((row[0] + row[1]) + row[2]) + row[3];
    }
    return ((wave[0] + wave[1]) + wave[2]) + wave[3];
}

/* ---- the 6 x 6 solve --------------------------------------------------------------------------------------------------------------- */
/* x = (H + lambda I)^-1 b by a dense Cholesky; H the upper triangle row by row (21); 0 on a non-positive or non-finite pivot */
int pr_solve6(const double *H, double lambda, const double *b, double *x)
{
    double A[36], L[36], y[6];
    int m = 0;
    for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) { A[a * 6 + c] = H[m]; A[c * 6 + a] = H[m]; ++m; }
    for (int a = 0; a < 6; ++a) A[a * 7] = A[a * 7] + lambda;
    for (int k = 0; k < 36; ++k) L[k] = 0.0;
    for (int j = 0; j < 6; ++j) {
        double d = A[j * 6 + j];
        for (int k = 0; k < j; ++k) d -= L[j * 6 + k] * L[j * 6 + k];
        if (!(d > 0 && d <= PR_DMAX)) return 0;
        const double ljj = sqrt(d);
        L[j * 6 + j] = ljj;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i * 6 + j];
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
    return 1;
}

/* ---- a frame ----------------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int n;
    const double *X, *obs;             /* [n][3], [n][3] */
    const int32_t *level;
    const uint8_t *kind;
    const uint8_t *outlier;            /* the flags of the previous classification */
    double K[5];                       /* fx fy cx cy bf */
} pr_frame;

/* one pass over the active edges at T: sum [28] (full) or sum [27] alone; *n_ok and *n_rej count the accepted and the rejected active edges.
 * d2m, d2s: the Huber widths of mono and stereo edges (<= 0: no kernel) */
static void pr_pass(const pr_frame *F, const double *T, int full, double d2m, double d2s, double *sum, int *n_ok, int *n_rej)
{
    static double lane[28][PR_LANES];
    double R[9];
    pr_rotation(T, R);
    const double dm = d2m > 0 ? sqrt(d2m) : 0.0, ds = d2s > 0 ? sqrt(d2s) : 0.0;
    *n_ok = 0; *n_rej = 0;
    for (int l = 0; l < PR_LANES; ++l) {
        double acc[28];
        for (int k = 0; k < 28; ++k) acc[k] = 0.0;
        for (int i = l; i < F->n; i += PR_LANES) {
            const int kind = F->kind[i];
            if (kind == 0 || F->outlier[i]) continue;
            const double d2 = kind == 2 ? d2s : d2m, delta = kind == 2 ? ds : dm;
            const int ok = full ? pr_edge_terms(R, T + 4, F->X + 3 * (size_t)i, F->obs + 3 * (size_t)i, F->level[i], kind, F->K, d2, delta, acc)
                                : pr_edge_cost(R, T + 4, F->X + 3 * (size_t)i, F->obs + 3 * (size_t)i, F->level[i], kind, F->K, d2, delta, acc);
            if (ok) ++*n_ok; else ++*n_rej;
        }
        for (int k = 0; k < 28; ++k) lane[k][l] = acc[k];
    }
    for (int k = full ? 0 : 27; k < 28; ++k) sum[k] = pr_reduce(lane[k]);
}

/* the stage for tests: the linearisation of all edges with kind != 0 at T: H [21], b [6] (= -J^T r), cost */
void pr_linearize(int n, const double *X, const double *obs, const int32_t *level, const uint8_t *kind, const double *K5, const double *T,
                  double d2m, double d2s, double *H, double *b, double *cost, int32_t *n_ok, int32_t *n_rej)
{
    uint8_t *out = (uint8_t *)calloc((size_t)(n > 0 ? n : 1), 1);
    pr_frame F = { n, X, obs, level, kind, out, { K5[0], K5[1], K5[2], K5[3], K5[4] } };
    double sum[28];
    int ok, rej;
    pr_pass(&F, T, 1, d2m, d2s, sum, &ok, &rej);
    for (int k = 0; k < 21; ++k) H[k] = sum[k];
    for (int k = 0; k < 6; ++k) b[k] = -sum[21 + k];
    *cost = sum[27]; *n_ok = ok; *n_rej = rej;
    free(out);
}

/* The whole call for one frame.  K4 = fx fy cx cy as doubles.  Outputs: pose_out [7]; outlier [n], chi2 [n] of the last classification (chi2 -1
 * for kind 0, 0 for a rejected edge); *inliers, *rounds_run; status, lm_iterations, cost_initial, cost_final, lambda [8] (unused rounds zero);
 * trace [trace_cap] (may be NULL) receives (round << 16 | iteration << 8 | code) per trial, *n_trace their number. */
void pr_optimize(const double *K4, int n, const double *X, const double *obs, const int32_t *level, const uint8_t *kind, const pr_params *prm,
                 const double *pose_in, double *pose_out, uint8_t *outlier, double *chi2, int32_t *inliers, int32_t *rounds_run,
                 int32_t *status, int32_t *lm_iterations, double *cost_initial, double *cost_final, double *lambda_out, int32_t *trace,
                 int trace_cap, int32_t *n_trace)
{
    pr_frame F = { n, X, obs, level, kind, outlier, { K4[0], K4[1], K4[2], K4[3], K4[0] * prm->baseline } };
    for (int i = 0; i < n; ++i) outlier[i] = 0;
    for (int k = 0; k < PR_MAX_ROUNDS; ++k) { status[k] = 0; lm_iterations[k] = 0; cost_initial[k] = 0.0; cost_final[k] = 0.0; lambda_out[k] = 0.0; }
    int nt = 0, inl = 0, run = 0;
    double T[7];
    memcpy(T, pose_in, sizeof T);
    for (int k = 0; k < prm->rounds; ++k) {
        const double d2m = k < prm->robust_rounds ? prm->chi2_mono : 0.0, d2s = k < prm->robust_rounds ? prm->chi2_stereo : 0.0;
        memcpy(T, pose_in, sizeof T);
        double lambda = 0.0, ni = 2.0, currentChi = 0.0;
        int st = PR_MAX_ITERATIONS, iters = 0;
        for (int it = 0; it < prm->iterations; ++it) {
            double sum[28], b[6];
            int n_ok, n_rej_lin;
            pr_pass(&F, T, 1, d2m, d2s, sum, &n_ok, &n_rej_lin);
            if (it == 0) {
                if (n_ok < prm->min_edges || !(fabs(sum[27]) <= PR_DMAX)) { st = PR_FAILED; break; }
                cost_initial[k] = sum[27];
            }
            currentChi = sum[27];
            for (int a = 0; a < 6; ++a) b[a] = -sum[21 + a];
            if (it == 0) {
                double mx = 0.0;
                int m = 0;
                for (int a = 0; a < 6; ++a) { const double h = fabs(sum[m]); if (h > mx) mx = h; m += 6 - a; }
                lambda = 1e-5 * mx; ni = 2.0;
            }
            double rho = 0.0;
            int qmax = 0, converged = 0;
            do {
                double d[6], Tn[7], tempChi = PR_DMAX, scale = 0.0;
                int ok = pr_solve6(sum, lambda, b, d);
                const int solved = ok;
                if (ok) {
                    int zero = 1;
                    for (int a = 0; a < 6; ++a) { zero &= d[a] == 0.0; scale += d[a] * (lambda * d[a] + b[a]); }
                    if (zero) memcpy(Tn, T, sizeof Tn);
                    else pr_retract(T, d, Tn);
                    double cs[28];
                    int c_ok, c_rej;
                    pr_pass(&F, Tn, 0, d2m, d2s, cs, &c_ok, &c_rej);
                    tempChi = cs[27];
                    ok = c_rej <= n_rej_lin && fabs(tempChi) <= PR_DMAX;
                    if (!ok) { tempChi = PR_DMAX; scale = 0.0; }
                }
                scale += 1e-3;
                rho = (currentChi - tempChi) / scale;
                if (!(fabs(rho) <= PR_DMAX)) rho = -1.0;
                const int accepted = ok && rho > 0;
                if (trace && nt < trace_cap) trace[nt] = (k << 16) | (it << 8) | (accepted ? PR_TRIAL_ACCEPTED : ok ? PR_TRIAL_REJECTED : solved ? PR_TRIAL_FAILED : PR_TRIAL_PIVOT);
                ++nt;
                if (accepted) {
                    const double u = 2.0 * rho - 1.0;
                    double alpha = 1.0 - u * u * u;
                    if (alpha > 2.0 / 3.0) alpha = 2.0 / 3.0;
                    lambda = lambda * (alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0);
                    ni = 2.0;
                    converged = currentChi - tempChi <= prm->min_rel_decrease * currentChi;
                    currentChi = tempChi;
                    memcpy(T, Tn, sizeof T);
                } else {
                    lambda = lambda * ni; ni = ni * 2.0;
                    if (!(fabs(lambda) <= PR_DMAX)) break;
                }
                ++qmax;
            } while (rho < 0 && qmax < prm->max_trials);
            ++iters;
            if (qmax == prm->max_trials || rho == 0 || !(fabs(lambda) <= PR_DMAX)) { st = PR_STALLED; break; }
            if (converged) { st = PR_CONVERGED; break; }
        }
        status[k] = st; lm_iterations[k] = iters; lambda_out[k] = lambda;
        cost_final[k] = st == PR_FAILED ? 0.0 : currentChi;
        /* classification of every edge with kind != 0 at the round's pose */
        double R[9];
        pr_rotation(T, R);
        inl = 0;
        for (int i = 0; i < n; ++i) {
            if (kind[i] == 0) { chi2[i] = -1.0; outlier[i] = 0; continue; }
            double P[3], r[3];
            if (!pr_residual(R, T + 4, X + 3 * (size_t)i, obs + 3 * (size_t)i, kind[i], F.K, P, r)) { chi2[i] = 0.0; outlier[i] = 1; continue; }
            const double c = pr_chi2(r, kind[i], pr_weight(level[i]));
            chi2[i] = c;
            outlier[i] = c > (kind[i] == 2 ? prm->chi2_stereo : prm->chi2_mono);
            inl += !outlier[i];
        }
        run = k + 1;
        if (inl < prm->min_inliers) break;
    }
    if (n_trace) *n_trace = nt;
    if (prm->rounds < 1) for (int i = 0; i < n; ++i) chi2[i] = kind[i] == 0 ? -1.0 : 0.0;
    memcpy(pose_out, T, sizeof T);
    *inliers = inl; *rounds_run = run;
}

/* the projection (u, v, uR) of X at T, for the scenes: the same operations as pr_residual; 0 behind the camera */
int pr_project(const double *K5, const double *T, const double *X, double *uvr)
{
    double R[9], P[3];
    pr_rotation(T, R);
    for (int i = 0; i < 3; ++i) P[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2]) + T[4 + i];
    if (!(P[2] > 0)) return 0;
    const double xn = P[0] / P[2], yn = P[1] / P[2], up = K5[0] * xn + K5[2];
    uvr[0] = up; uvr[1] = K5[1] * yn + K5[3]; uvr[2] = up - K5[4] / P[2];
    return 1;
}
