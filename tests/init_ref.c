/* init_ref.c -- restatement of the reference's monocular Initializer (src/Algorithm/Initializer.cpp), the yardstick of
 * ygz_slam_amd/csrc/init.hip (tests/test_init_ref.py, tests/test_gpu_initializer.py).  Test infrastructure: plain C99, single-threaded,
 * built by tests/init_ref.py with -O2 -ffp-contract=off -fno-fast-math and never linked into the product.
 *
 * Every function cites the lines it restates and keeps the reference's float / double promotions as written.  Where the reference
 * leans on Eigen / OpenCV / Sophus internals the restatement states its own algorithm:
 *  - cv::RNG (default seed 0xffffffff, multiply-with-carry, uniform(int,int) = next() % (b - a) + a): parity unpinned;
 *  - every SVD is one-sided (Hestenes) Jacobi on the matrix itself (ir_jacobi), fixed cyclic pair order, stated stop rule;
 *  - 3x3 inverse / determinant in cofactor form; matrix products and dot products summed left to right;
 *  - undefined behaviour of the reference made definite: Normalize's accumulators start at 0, "no hypothesis scored" is reported
 *    as no model, p3D of rejected points is 0, R21 / t21 of a failed reconstruction are I / 0. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* the result block; the same layout as ygz_init_result (include/ygz_hip.h) */
typedef struct {
    double  H21[9], F21[9];
    double  R21[9], t21[3];
    double  T21[7];
    double  parallax;
    float   score_h, score_f, rh;
    int32_t success, model, best_h, best_f;
    int32_t n_inliers, solution, n_good, second_good, similar, n_triangulated;
} ir_result;

enum { IR_NONE = 0, IR_H = 1, IR_F = 2 };

/* ---- cv::RNG (OpenCV core/operations.hpp: RNG::next, RNG::uniform(int,int); default state 0xffffffff) --------------------- */
static uint32_t rng_next(uint64_t *s)
{
    *s = (uint64_t)(uint32_t)*s * 4164903690u + (uint32_t)(*s >> 32);
    return (uint32_t)*s;
}

/* TryInitialize :24-48 -- the 8 distinct indices of every iteration, drawn from a fresh cv::RNG (so they depend on n and max_iter only) */
void ir_sample_sets(int n, int max_iter, int32_t *sets)
{
    uint64_t st = 0xffffffffu;
    int32_t avail[n > 0 ? n : 1];
    for (int it = 0; it < max_iter; ++it) {
        int na = n;
        for (int i = 0; i < n; ++i) avail[i] = i;
        for (int j = 0; j < 8; ++j) {
            const int a = 0, b = na;                                 /* rng.uniform(0, availableIndices.size()): the int overload */
            const int r = a == b ? a : (int)(rng_next(&st) % (uint32_t)(b - a) + (uint32_t)a);
            sets[it * 8 + j] = avail[r];
            avail[r] = avail[na - 1];
            --na;
        }
    }
}

/* ---- one-sided Jacobi SVD ----------------------------------------------------------------------------------------------------
 * A (m x n, row-major, element (i,j) at A[(i*n + j)*st]) is replaced by W = A V with mutually orthogonal columns; V (n x n, same
 * stride) accumulates the rotations.  Sweeps visit the pairs (p, q), p < q, row by row; a pair is rotated when
 * |gamma| > 1e-15 * sqrt(alpha) * sqrt(beta) (alpha, beta, gamma summed over the rows in index order); at most 40 sweeps, and a sweep
 * without a rotation ends the loop.  The rotation is Rutishauser's: zeta = (beta - alpha) / (2 gamma),
 * t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) (t = 1 / (2 zeta) when |zeta| > 1e150), c = 1 / sqrt(1 + t^2), s = c t. */
#define IR_JACOBI_TOL 1e-15
#define IR_JACOBI_SWEEPS 40
void ir_jacobi(double *A, int m, int n, double *V, int st)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[(i * n + j) * st] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < IR_JACOBI_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int i = 0; i < m; ++i) {
                    const double ap = A[(i * n + p) * st], aq = A[(i * n + q) * st];
                    alpha = alpha + ap * ap; beta = beta + aq * aq; gamma = gamma + ap * aq;
                }
                if (!(fabs(gamma) > IR_JACOBI_TOL * sqrt(alpha) * sqrt(beta))) continue;
                rotated = 1;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                double t;
                if (fabs(zeta) > 1e150) t = 1.0 / (2.0 * zeta);
                else t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < m; ++i) {
                    const double ap = A[(i * n + p) * st], aq = A[(i * n + q) * st];
                    A[(i * n + p) * st] = c * ap - s * aq;
                    A[(i * n + q) * st] = s * ap + c * aq;
                }
                for (int i = 0; i < n; ++i) {
                    const double vp = V[(i * n + p) * st], vq = V[(i * n + q) * st];
                    V[(i * n + p) * st] = c * vp - s * vq;
                    V[(i * n + q) * st] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
}

/* column norms of W after ir_jacobi = the singular values; ord[] lists the columns by decreasing norm (ties: lower index first) */
void ir_sv_order(const double *W, int m, int n, int st, double *sv, int *ord)
{
    for (int j = 0; j < n; ++j) {
        double s = 0;
        for (int i = 0; i < m; ++i) { const double w = W[(i * n + j) * st]; s = s + w * w; }
        sv[j] = sqrt(s);
        ord[j] = j;
    }
    for (int a = 1; a < n; ++a)                                      /* insertion sort: stable */
        for (int b = a; b > 0 && sv[ord[b]] > sv[ord[b - 1]]; --b) { const int t = ord[b]; ord[b] = ord[b - 1]; ord[b - 1] = t; }
}

/* the right singular vector of the smallest singular value of A (m x n), into x[n] (A is overwritten): the column of W whose norm is
 * <= every earlier one's, the last such (what a stable decreasing sort puts last) */
void ir_null_vector(double *A, int m, int n, double *V, double *x)
{
    double sv[9]; int ord[9], c = 0;
    ir_jacobi(A, m, n, V, 1);
    ir_sv_order(A, m, n, 1, sv, ord);
    for (int j = 0; j < n; ++j) if (j == 0 || sv[j] <= sv[c]) c = j;
    for (int i = 0; i < n; ++i) x[i] = V[i * n + c];
}

/* full SVD of a 3x3 (row-major): A = U diag(s) V^T, s decreasing, u3 = u1 x u2 (det U = +1; v3 flipped when A v3 points the other
 * way, so the product still equals A) */
void ir_svd3(const double *A, double *U, double *s, double *V)
{
    double W[9], Vj[9], sv[3]; int ord[3];
    memcpy(W, A, sizeof W);
    ir_jacobi(W, 3, 3, Vj, 1);
    ir_sv_order(W, 3, 3, 1, sv, ord);
    for (int k = 0; k < 3; ++k) {
        s[k] = sv[ord[k]];
        for (int i = 0; i < 3; ++i) V[i * 3 + k] = Vj[i * 3 + ord[k]];
    }
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < 3; ++i) U[i * 3 + k] = W[i * 3 + ord[k]] / s[k];
    U[0 * 3 + 2] = U[1 * 3 + 0] * U[2 * 3 + 1] - U[2 * 3 + 0] * U[1 * 3 + 1];
    U[1 * 3 + 2] = U[2 * 3 + 0] * U[0 * 3 + 1] - U[0 * 3 + 0] * U[2 * 3 + 1];
    U[2 * 3 + 2] = U[0 * 3 + 0] * U[1 * 3 + 1] - U[1 * 3 + 0] * U[0 * 3 + 1];
    const double d = U[0 * 3 + 2] * W[0 * 3 + ord[2]] + U[1 * 3 + 2] * W[1 * 3 + ord[2]] + U[2 * 3 + 2] * W[2 * 3 + ord[2]];
    if (d < 0)
        for (int i = 0; i < 3; ++i) V[i * 3 + 2] = -V[i * 3 + 2];
}

/* ---- 3x3 helpers (row-major) -------------------------------------------------------------------------------------------------- */
static void mul3(const double *a, const double *b, double *r)        /* r = a b, sums left to right */
{
    double t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[i * 3 + j] = a[i * 3 + 0] * b[0 * 3 + j] + a[i * 3 + 1] * b[1 * 3 + j] + a[i * 3 + 2] * b[2 * 3 + j];
    memcpy(r, t, sizeof t);
}
static void mul3t(const double *a, const double *b, double *r)       /* r = a b^T */
{
    double t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[i * 3 + j] = a[i * 3 + 0] * b[j * 3 + 0] + a[i * 3 + 1] * b[j * 3 + 1] + a[i * 3 + 2] * b[j * 3 + 2];
    memcpy(r, t, sizeof t);
}
static void tr3(const double *a, double *r) { for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r[i * 3 + j] = a[j * 3 + i]; }
double ir_det3(const double *a)                                      /* cofactor expansion along the first row */
{
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    return a[0] * c0 + a[1] * c1 + a[2] * c2;
}
/* on the device: ygz_inv3 (ygz_slam_amd/csrc/posemath_dev.h) */
void ir_inv3(const double *a, double *r)                             /* adj(a) * (1 / det), det = a00 C00 + a01 C01 + a02 C02 */
{
    double C[9];
    C[0] = a[4] * a[8] - a[5] * a[7]; C[1] = a[5] * a[6] - a[3] * a[8]; C[2] = a[3] * a[7] - a[4] * a[6];
    C[3] = a[2] * a[7] - a[1] * a[8]; C[4] = a[0] * a[8] - a[2] * a[6]; C[5] = a[1] * a[6] - a[0] * a[7];
    C[6] = a[1] * a[5] - a[2] * a[4]; C[7] = a[2] * a[3] - a[0] * a[5]; C[8] = a[0] * a[4] - a[1] * a[3];
    const double det = a[0] * C[0] + a[1] * C[1] + a[2] * C[2];
    const double inv = 1.0 / det;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r[i * 3 + j] = C[j * 3 + i] * inv;
}

/* Sophus SO3(const Matrix3d &) = Eigen's quaternion-from-matrix (trace branch, else the largest diagonal); q = (x, y, z, w) */
/* on the device: ygz_quat_from_matrix (ygz_slam_amd/csrc/posemath_dev.h) */
void ir_quat_from_matrix(const double *m, double *q)
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

/* ---- Normalize :140-175 (mean and meanDev start at 0: the reference leaves them uninitialised) -------------------------------- */
void ir_normalize(const double *px, int n, double *pn, double *T)
{
    double m0 = 0, m1 = 0;
    for (int i = 0; i < n; ++i) { m0 = m0 + px[2 * i]; m1 = m1 + px[2 * i + 1]; }
    m0 = m0 / (double)n; m1 = m1 / (double)n;
    double d0 = 0, d1 = 0;
    for (int i = 0; i < n; ++i) {
        pn[2 * i] = px[2 * i] - m0; pn[2 * i + 1] = px[2 * i + 1] - m1;
        d0 = d0 + fabs(pn[2 * i]); d1 = d1 + fabs(pn[2 * i + 1]);
    }
    d0 = d0 / (double)n; d1 = d1 / (double)n;
    const float sX = 1.0 / d0, sY = 1.0 / d1;
    for (int i = 0; i < n; ++i) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
    T[0] = sX; T[1] = 0; T[2] = -m0 * sX;
    T[3] = 0; T[4] = sY; T[5] = -m1 * sY;
    T[6] = 0; T[7] = 0; T[8] = 1;
}

/* ---- ComputeH21 :196-239 / ComputeF21 :730-762 (pn1i, pn2i: the 8 sampled normalised points) ---------------------------------- */
void ir_compute_h21(const double *p1, const double *p2, double *H)
{
    double A[16 * 9], V[81], x[9];
    for (int i = 0; i < 8; ++i) {
        const double u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        double *r0 = A + (2 * i) * 9, *r1 = A + (2 * i + 1) * 9;
        r0[0] = 0.0; r0[1] = 0.0; r0[2] = 0.0; r0[3] = -u1; r0[4] = -v1; r0[5] = -1; r0[6] = v2 * u1; r0[7] = v2 * v1; r0[8] = v2;
        r1[0] = u1; r1[1] = v1; r1[2] = 1; r1[3] = 0.0; r1[4] = 0.0; r1[5] = 0.0; r1[6] = -u2 * u1; r1[7] = -u2 * v1; r1[8] = -u2;
    }
    ir_null_vector(A, 16, 9, V, x);
    for (int k = 0; k < 9; ++k) H[k] = x[k];
}

void ir_compute_f21(const double *p1, const double *p2, double *F)
{
    double A[8 * 9], V[81], x[9];
    for (int i = 0; i < 8; ++i) {
        const double u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        double *r = A + i * 9;
        r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1;
    }
    ir_null_vector(A, 8, 9, V, x);
    double U[9], s[3], Vf[9], UD[9];
    ir_svd3(x, U, s, Vf);                                            /* :759-761: U diag(s0, s1, 0) V^T */
    for (int i = 0; i < 3; ++i) { UD[i * 3 + 0] = U[i * 3 + 0] * s[0]; UD[i * 3 + 1] = U[i * 3 + 1] * s[1]; UD[i * 3 + 2] = U[i * 3 + 2] * 0.0; }
    mul3t(UD, Vf, F);
}

/* ---- CheckHomography :251-314 (one direction: image 2 into image 1) ---------------------------------------------------------- */
float ir_h_contrib(const double *H12, const double *px1, const double *px2, int i, float invSigmaSquare, int *in)
{
    const float th = 5.991;
    const double u1 = px1[2 * i], v1 = px1[2 * i + 1], u2 = px2[2 * i], v2 = px2[2 * i + 1];
    const float w2in1inv = 1.0 / (H12[6] * u2 + H12[7] * v2 + H12[8]);
    const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
    const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { *in = 0; return 0.0f; }
    *in = 1;
    return th - chiSquare1;
}

/* ---- CheckFundamental :772-845 (all float; both directions, thScore per direction) ------------------------------------------ */
void ir_f_contrib(const float *f, const double *px1, const double *px2, int i, float invSigmaSquare, float *c1, float *c2, int *in)
{
    const float th = 3.841, thScore = 5.991;
    const float u1 = px1[2 * i], v1 = px1[2 * i + 1], u2 = px2[2 * i], v2 = px2[2 * i + 1];
    int bIn = 1;
    const float a2 = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2_ = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2_;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = 0; *c1 = 0.0f; } else *c1 = thScore - chiSquare1;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1_ = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1_;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = 0; *c2 = 0.0f; } else *c2 = thScore - chiSquare2;
    *in = bIn;
}

/* ---- FindHomography :89-138 / FindFundamental :670-718: every hypothesis' model and score, and the winners (first strict
 * maximum above 0; -1 when none scored above 0, the reference then never assigns H21 / F21) ------------------------------------- */
void ir_hypotheses(const double *px1, const double *px2, int n, const int32_t *sets, int max_iter, float sigma,
                   double *H21all, double *F21all, float *score_h, float *score_f, ir_result *res, uint8_t *inl_h, uint8_t *inl_f)
{
    double pn1[2 * n], pn2[2 * n], T1[9], T2[9], T2inv[9], T2t[9];
    ir_normalize(px1, n, pn1, T1);
    ir_normalize(px2, n, pn2, T2);
    ir_inv3(T2, T2inv);
    tr3(T2, T2t);
    const float invSigmaSquare = 1.0 / (sigma * sigma);
    float bh = 0, bf = 0;
    int ih = -1, jf = -1;
    for (int it = 0; it < max_iter; ++it) {
        double p1[16], p2[16], Hn[9], Fn[9], H[9], H12[9], F[9];
        for (int j = 0; j < 8; ++j) {
            const int idx = sets[it * 8 + j];
            p1[2 * j] = pn1[2 * idx]; p1[2 * j + 1] = pn1[2 * idx + 1];
            p2[2 * j] = pn2[2 * idx]; p2[2 * j + 1] = pn2[2 * idx + 1];
        }
        ir_compute_h21(p1, p2, Hn);
        mul3(T2inv, Hn, H); mul3(H, T1, H);
        ir_inv3(H, H12);
        ir_compute_f21(p1, p2, Fn);
        mul3(T2t, Fn, F); mul3(F, T1, F);
        float sh = 0, sf = 0, fl[9];
        for (int k = 0; k < 9; ++k) fl[k] = F[k];
        for (int i = 0; i < n; ++i) {
            int in;
            sh += ir_h_contrib(H12, px1, px2, i, invSigmaSquare, &in);
            float c1, c2;
            ir_f_contrib(fl, px1, px2, i, invSigmaSquare, &c1, &c2, &in);
            sf += c1;
            sf += c2;
        }
        if (H21all) memcpy(H21all + 9 * it, H, sizeof H);
        if (F21all) memcpy(F21all + 9 * it, F, sizeof F);
        if (score_h) score_h[it] = sh;
        if (score_f) score_f[it] = sf;
        if (sh > bh) { bh = sh; ih = it; memcpy(res->H21, H, sizeof H); }
        if (sf > bf) { bf = sf; jf = it; memcpy(res->F21, F, sizeof F); }
    }
    res->score_h = bh; res->score_f = bf; res->best_h = ih; res->best_f = jf;
    /* the winners' inlier masks (all false when nothing won: vbMatchesInliers = vector<bool>(_num_points, false)) */
    double H12[9];
    float fl[9];
    if (ih >= 0) ir_inv3(res->H21, H12);
    for (int k = 0; k < 9; ++k) fl[k] = res->F21[k];
    for (int i = 0; i < n; ++i) {
        int in = 0;
        if (ih >= 0) (void)ir_h_contrib(H12, px1, px2, i, invSigmaSquare, &in);
        inl_h[i] = (uint8_t)in;
        in = 0;
        float c1, c2;
        if (jf >= 0) ir_f_contrib(fl, px1, px2, i, invSigmaSquare, &c1, &c2, &in);
        inl_f[i] = (uint8_t)in;
    }
    /* TryInitialize :66-78: rh in float, H when rh > 0.4; sh + sf == 0 (rh NaN): no model */
    res->rh = bh / (bh + bf);
    res->model = (bh + bf == 0) ? IR_NONE : (res->rh > 0.4 ? IR_H : IR_F);
}

/* ---- Triangulate :649-662 ----------------------------------------------------------------------------------------------------- */
void ir_triangulate(const double *kp1, const double *kp2, const double *P1, const double *P2, double *x3D)
{
    double A[16], V[16], x[4];
    for (int c = 0; c < 4; ++c) {
        A[0 * 4 + c] = kp1[0] * P1[2 * 4 + c] - P1[0 * 4 + c];
        A[1 * 4 + c] = kp1[1] * P1[2 * 4 + c] - P1[1 * 4 + c];
        A[2 * 4 + c] = kp2[0] * P2[2 * 4 + c] - P2[0 * 4 + c];
        A[3 * 4 + c] = kp2[1] * P2[2 * 4 + c] - P2[1 * 4 + c];
    }
    ir_null_vector(A, 4, 4, V, x);
    x3D[0] = x[0] / x[3]; x3D[1] = x[1] / x[3]; x3D[2] = x[2] / x[3];
}

/* P1 = K [I | 0], P2 = K [R | t] (3 x 4 row-major), O2 = -R^T t (:522-532) */
void ir_cameras(const double *K, const double *R, const double *t, double *P1, double *P2, double *O2)
{
    double Rt[12];
    memset(P1, 0, 12 * sizeof(double));
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { P1[i * 4 + j] = K[i * 3 + j]; Rt[i * 4 + j] = R[i * 3 + j]; }
    for (int i = 0; i < 3; ++i) Rt[i * 4 + 3] = t[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) P2[i * 4 + j] = K[i * 3 + 0] * Rt[0 * 4 + j] + K[i * 3 + 1] * Rt[1 * 4 + j] + K[i * 3 + 2] * Rt[2 * 4 + j];
    for (int i = 0; i < 3; ++i) O2[i] = -R[0 * 3 + i] * t[0] + -R[1 * 3 + i] * t[1] + -R[2 * 3 + i] * t[2];
}

/* ---- CheckRT :505-616, one point: returns 1 when the point counts (cntGood), *good when also cosParallax < 0.99998 ------------ */
int ir_checkrt_point(const double *R, const double *t, const double *K, const double *P1, const double *P2, const double *O2,
                     const double *px1, const double *px2, int i, float th2, int check_reproj, double *p3d, int *good, float *cosp)
{
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    double p[3];
    *good = 0;
    ir_triangulate(px1 + 2 * i, px2 + 2 * i, P1, P2, p);
    if (!isfinite(p[0])) return 0;
    const double n2x = p[0] - O2[0], n2y = p[1] - O2[1], n2z = p[2] - O2[2];
    const double dist1 = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const double dist2 = sqrt(n2x * n2x + n2y * n2y + n2z * n2z);
    const double cosParallax = (p[0] * n2x + p[1] * n2y + p[2] * n2z) / (dist1 * dist2);
    if (p[2] < 0 && cosParallax < 0.99998) return 0;
    double q[3];
    for (int r = 0; r < 3; ++r) q[r] = R[r * 3 + 0] * p[0] + R[r * 3 + 1] * p[1] + R[r * 3 + 2] * p[2] + t[r];
    if (q[2] < 0 && cosParallax < 0.99998) return 0;
    if (check_reproj) {
        const double invZ1 = 1.0 / p[2];
        const double im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
        const double e1 = (im1x - px1[2 * i]) * (im1x - px1[2 * i]) + (im1y - px1[2 * i + 1]) * (im1y - px1[2 * i + 1]);
        if (e1 > th2) return 0;
        const double invZ2 = 1.0 / q[2];
        const double im2x = fx * q[0] * invZ2 + cx, im2y = fy * q[1] * invZ2 + cy;
        const double e2 = (im2x - px2[2 * i]) * (im2x - px2[2 * i]) + (im2y - px2[2 * i + 1]) * (im2y - px2[2 * i + 1]);
        if (e2 > th2) return 0;
    }
    *cosp = (float)cosParallax;
    p3d[0] = p[0]; p3d[1] = p[1]; p3d[2] = p[2];
    if (cosParallax < 0.99998) *good = 1;
    return 1;
}

/* :607-614: the (min(50, count - 1))-th smallest of the counted points' float cosParallax after the sort; NaN when one of them is NaN
 * (std::sort's order is unspecified for NaN).  Then acos of the float, in float (acos(float) is std::acos(float) under the reference's
 * `using namespace std`): restated as the double acos rounded to float, times 180 in float, over M_PI. */
static int cmp_float(const void *a, const void *b)
{
    const float x = *(const float *)a, y = *(const float *)b;
    return x < y ? -1 : (y < x ? 1 : 0);
}
double ir_parallax(const float *cosv, const uint8_t *counted, int n, int cnt)
{
    if (cnt <= 0) return 0;
    const int idx = cnt - 1 < 50 ? cnt - 1 : 50;
    float v[cnt];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        if (!counted[i]) continue;
        if (isnan(cosv[i])) return NAN;
        v[m++] = cosv[i];
    }
    qsort(v, (size_t)m, sizeof(float), cmp_float);
    const float a = (float)acos((double)v[idx]);
    return (double)(a * 180.0f) / M_PI;
}

/* CheckRT over all points for one (R, t): count, parallax, p3D (0 where not counted), good mask */
int ir_checkrt(const double *R, const double *t, const double *K, const double *px1, const double *px2, int n, float th2, int check_reproj,
               double *p3d, uint8_t *good, double *parallax)
{
    double P1[12], P2[12], O2[3];
    float cosv[n > 0 ? n : 1];
    uint8_t counted[n > 0 ? n : 1];
    ir_cameras(K, R, t, P1, P2, O2);
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        int g;
        p3d[3 * i] = p3d[3 * i + 1] = p3d[3 * i + 2] = 0;
        cosv[i] = 0;
        counted[i] = (uint8_t)ir_checkrt_point(R, t, K, P1, P2, O2, px1, px2, i, th2, check_reproj, p3d + 3 * i, &g, cosv + i);
        good[i] = (uint8_t)g;
        cnt += counted[i];
    }
    *parallax = ir_parallax(cosv, counted, n, cnt);
    return cnt;
}

/* ---- ReconstructH :326-503 -- the 8 Faugeras solutions; returns 0 when d1/d2 or d2/d3 < 1.00001 (no solutions) --------------- */
int ir_h_solutions(const double *H21, const double *K, double *Rs, double *ts)
{
    double invK[9], A[9], U[9], sg[3], V[9];
    ir_inv3(K, invK);
    mul3(invK, H21, A); mul3(A, K, A);
    ir_svd3(A, U, sg, V);
    const double d1 = sg[0], d2 = sg[1], d3 = sg[2];
    const double s = ir_det3(U) * ir_det3(V);
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return 0;
    const float aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[] = { aux1, aux1, -aux1, -aux1 };
    const float x3[] = { aux3, -aux3, aux3, -aux3 };
    const float aux_stheta = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[] = { aux_stheta, -aux_stheta, -aux_stheta, aux_stheta };
    const float aux_sphi = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[] = { aux_sphi, -aux_sphi, -aux_sphi, aux_sphi };
    double sU[9];
    for (int k = 0; k < 9; ++k) sU[k] = s * U[k];
    for (int i = 0; i < 8; ++i) {
        double Rp[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 }, tp[3], *R = Rs + 9 * i, *t = ts + 3 * i;
        if (i < 4) {                                                 /* :385-412, case d' = d2 */
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp[0] = x1[i]; tp[1] = 0.0; tp[2] = -x3[i];
            for (int k = 0; k < 3; ++k) tp[k] = tp[k] * (d1 - d3);
        } else {                                                     /* :418-449, case d' = -d2 */
            const int j = i - 4;
            Rp[0] = cphi; Rp[2] = sphi[j]; Rp[4] = -1; Rp[6] = sphi[j]; Rp[8] = -cphi;
            tp[0] = x1[j]; tp[1] = 0; tp[2] = x3[j];
            for (int k = 0; k < 3; ++k) tp[k] = tp[k] * (d1 + d3);
        }
        mul3(sU, Rp, R); mul3t(R, V, R);
        for (int r = 0; r < 3; ++r) t[r] = U[r * 3 + 0] * tp[0] + U[r * 3 + 1] * tp[1] + U[r * 3 + 2] * tp[2];
        const double nr = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
        for (int r = 0; r < 3; ++r) t[r] = t[r] / nr;
    }
    return 1;
}

/* ---- DecomposeE :940-963 -------------------------------------------------------------------------------------------------------- */
void ir_decompose_e(const double *E, double *R1, double *R2, double *t)
{
    double U[9], s[3], V[9], UW[9];
    ir_svd3(E, U, s, V);
    for (int i = 0; i < 3; ++i) t[i] = U[i * 3 + 2];
    const double nr = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int i = 0; i < 3; ++i) t[i] = t[i] / nr;
    const double W[9] = { 0, -1, 0, 1, 0, 0, 0, 0, 1 }, Wt[9] = { 0, 1, 0, -1, 0, 0, 0, 0, 1 };
    mul3(U, W, UW); mul3t(UW, V, R1);
    if (ir_det3(R1) < 0) for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
    mul3(U, Wt, UW); mul3t(UW, V, R2);
    if (ir_det3(R2) < 0) for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
}

/* the candidate motions of a model: 8 (H, :385-449) or 4 (F, :856-877: (R1, t), (R2, t), (R1, -t), (R2, -t)); 0 when H is degenerate */
int ir_solutions(int model, const double *M, const double *K, double *Rs, double *ts)
{
    if (model == IR_H) return ir_h_solutions(M, K, Rs, ts) ? 8 : 0;
    double Kt[9], E[9], R1[9], R2[9], t[3];
    tr3(K, Kt);
    mul3(Kt, M, E); mul3(E, K, E);
    ir_decompose_e(E, R1, R2, t);
    for (int k = 0; k < 9; ++k) { Rs[k] = R1[k]; Rs[9 + k] = R2[k]; Rs[18 + k] = R1[k]; Rs[27 + k] = R2[k]; }
    for (int k = 0; k < 3; ++k) { ts[k] = t[k]; ts[3 + k] = t[k]; ts[6 + k] = -t[k]; ts[9 + k] = -t[k]; }
    return 4;
}

/* ---- ReconstructH :451-501 / ReconstructF :852-937 from a given model; res gets solution, n_good, second_good, similar, parallax,
 * success, R21 / t21 / T21 (I / 0 unless accepted), n_triangulated; p3d [n][3] and tri [n] of the accepted solution (0 otherwise) */
void ir_reconstruct(const double *px1, const double *px2, int n, const double *K4, int model, const double *M, const uint8_t *inliers,
                    float sigma2, double min_parallax_d, int min_triangulated, double ratio_h, ir_result *res, double *p3d, uint8_t *tri)
{
    const double K[9] = { K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1 };
    const float minParallax = (float)min_parallax_d;
    double Rs[72], ts[24];
    int N = 0;
    for (int i = 0; i < n; ++i) N += inliers[i] != 0;
    res->n_inliers = N; res->model = model;
    res->success = 0; res->solution = -1; res->n_good = 0; res->second_good = 0; res->similar = 0; res->parallax = 0; res->n_triangulated = 0;
    memset(p3d, 0, (size_t)n * 3 * sizeof(double));
    memset(tri, 0, (size_t)n);
    const int ns = (model == IR_H || model == IR_F) ? ir_solutions(model, M, K, Rs, ts) : 0;
    double par[8];
    int good[8];
    double sp3d[3 * (n > 0 ? n : 1)];
    uint8_t sgood[n > 0 ? n : 1];
    for (int k = 0; k < ns; ++k)
        good[k] = ir_checkrt(Rs + 9 * k, ts + 3 * k, K, px1, px2, n, model == IR_H ? (float)(4.0 * sigma2) : (float)(24.0 * sigma2),
                             model == IR_H, sp3d, sgood, par + k);
    int best = -1, accept = 0;
    if (model == IR_H && ns == 8) {
        int bestGood = 0, secondBestGood = 0;
        float bestParallax = -1;
        for (int i = 0; i < 8; ++i) {
            if (good[i] > bestGood) { secondBestGood = bestGood; bestGood = good[i]; best = i; bestParallax = par[i]; }
            else if (good[i] > secondBestGood) secondBestGood = good[i];
        }
        res->n_good = bestGood; res->second_good = secondBestGood;
        res->parallax = best >= 0 ? par[best] : 0;
        accept = secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > min_triangulated && bestGood > ratio_h * n;
    } else if (model == IR_F) {
        int maxGood = good[0];
        for (int i = 1; i < 4; ++i) if (good[i] > maxGood) maxGood = good[i];
        const int ng = (int)(0.9 * N), minGood = ng > min_triangulated ? ng : min_triangulated;
        int similar = 0, second = 0;
        for (int i = 0; i < 4; ++i) if (good[i] > 0.7 * maxGood) ++similar;
        for (int i = 0; i < 4; ++i) if (best < 0 && good[i] == maxGood) best = i;      /* first listed */
        for (int i = 0; i < 4; ++i) if (i != best && good[i] > second) second = good[i];
        res->n_good = maxGood; res->second_good = second; res->similar = similar; res->parallax = par[best];
        accept = !(maxGood < minGood || similar > 1) && par[best] > minParallax;
    }
    res->solution = best;
    for (int k = 0; k < 9; ++k) res->R21[k] = (k % 4 == 0) ? 1.0 : 0.0;
    for (int k = 0; k < 3; ++k) res->t21[k] = 0;
    if (accept) {
        res->success = 1;
        memcpy(res->R21, Rs + 9 * best, 9 * sizeof(double));
        memcpy(res->t21, ts + 3 * best, 3 * sizeof(double));
        double par_;
        (void)ir_checkrt(Rs + 9 * best, ts + 3 * best, K, px1, px2, n, model == IR_H ? (float)(4.0 * sigma2) : (float)(24.0 * sigma2),
                         model == IR_H, p3d, tri, &par_);
        for (int i = 0; i < n; ++i) res->n_triangulated += tri[i];
    }
    ir_quat_from_matrix(res->R21, res->T21);                         /* _T21 = SE3(R21, t21) (:79) */
    for (int k = 0; k < 3; ++k) res->T21[4 + k] = res->t21[k];
}

/* ---- TryInitialize :9-87 ------------------------------------------------------------------------------------------------------- */
int ir_initialize(const double *px1, const double *px2, int n, const double *K4, float sigma, float sigma2, int max_iter, double min_parallax,
                  int min_triangulated, double ratio_h, ir_result *res, double *p3d, uint8_t *tri)
{
    memset(res, 0, sizeof *res);
    int32_t sets[8 * max_iter];
    uint8_t inl_h[n], inl_f[n];
    ir_sample_sets(n, max_iter, sets);
    ir_hypotheses(px1, px2, n, sets, max_iter, sigma, 0, 0, 0, 0, res, inl_h, inl_f);
    const int model = res->model;
    ir_reconstruct(px1, px2, n, K4, model, model == IR_H ? res->H21 : res->F21, model == IR_H ? inl_h : inl_f, sigma2, min_parallax,
                   min_triangulated, ratio_h, res, p3d, tri);
    return res->success;
}
