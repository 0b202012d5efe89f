/* Restatement of the pyramidal Lucas-Kanade tracker (ygz_slam_amd/csrc/klt.hip: k_klt3, k_klt<false> and their host code) in plain C99.
 * TEST INFRASTRUCTURE: built by tests/klt_ref.py with gcc -O2 -ffp-contract=off -fno-fast-math into a temporary directory, never linked
 * into the package.
 *
 * Every integer term, weight, decision and level rule is that of oracle/klt.c (the generic path of OpenCV's lkpyramid.cpp); the caller
 * hands in the pyramid levels (oracle pyrDown), and this file applies buildOpticalFlowPyramid's stop rule, the REFLECT_101 frame of
 * the images, the zero frame of the Scharr images, and the tracker with ygz_klt_params' fields and clamps.  The ONE thing that differs
 * between the oracle and the two kernels is the association of five float sums per evaluation -- A11, A12, A22, b1 / b2, and the
 * error -- which `order` selects:
 *   0  sequential: all win * win terms converted to float and added in raster order (oracle/klt.c);
 *   1  k_klt3 (win 21): a window belongs to 21 lanes q = 0..20, lane q owns rows 3 (q / 3) .. + 2 and columns 7 (q % 3) .. + 6.  A lane
 *      adds its 21 integer products exactly in int32 and converts once; for the error it adds fabsf((float)diff) in float from 0.f,
 *      rows outer, columns inner.  The 21 lane values: v[q] += v[q + 16] (q < 5), += v[q + 8] (q < 8), += v[q + 4] (q < 4),
 *      += v[q + 2] (q < 2), result v[0] + v[1];
 *   2  k_klt<false> (win 3..20): lane l of 64 has row l / 3 and first column 7 (l % 3), is active when row < win and column < win,
 *      and owns min(7, win - column) pixels; lane sums as in order 1, idle lanes 0.f; then ygz_wave_sum_f's association
 *      (ygz_internal.h): quad xor 1, quad xor 2, half-row mirror, row mirror, then rows 0..3 left to right.
 * An int64 shadow of every int32 lane sum is kept; kr_track returns KR_E_OVERFLOW if they ever differ.
 *
 * Taps, per point and level (arrays [n][KR_MAX_LEVELS]; level slots the track never visits stay KR_NOT_RUN / 0):
 *   exit      which way the level ended (KR_*), iters the number of mismatch evaluations (for KR_GUESS_OUT: the iteration j at which
 *             the window was found outside), min_eig the eigenvalue that was tested, in the selected order;
 *   max_sum   [n] the largest magnitude of any partial sum (lane value or intermediate) of the point's float sums. */
#include <math.h>
#include <float.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define KR_MAX_LEVELS 8
enum { KR_NOT_RUN = 0, KR_REF_OUT, KR_EIG_FAIL, KR_GUESS_OUT, KR_CONVERGED, KR_OSCILLATION, KR_MAX_ITER, KR_ERR_OUT };
enum { KR_OK = 0, KR_E_INVALID = -1, KR_E_LEVELS = -2, KR_E_OVERFLOW = -3 };

typedef struct { int win, max_level, max_iter; double eps, min_eig_threshold; int use_initial_flow; } kr_params;   /* ygz_klt_params */

typedef struct { int w, h; const uint8_t *img; int16_t *deriv; /* [h][w][2] */ } kr_level;

static int refl101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}
/* the image inside its REFLECT_101 frame */
static int I_at(const kr_level *L, int x, int y) { return L->img[(size_t)refl101(y, L->h) * L->w + refl101(x, L->w)]; }
/* the Scharr image inside its zero frame */
static int D_at(const kr_level *L, int x, int y, int c)
{
    if (x < 0 || y < 0 || x >= L->w || y >= L->h) return 0;
    return L->deriv[((size_t)y * L->w + x) * 2 + c];
}
/* calcSharrDeriv: 3/10/3 smoothing across, central difference along; REFLECT_101 at the image's edge */
static void scharr(kr_level *L)
{
    const int w = L->w, h = L->h;
    L->deriv = (int16_t *)malloc(sizeof(int16_t) * 2 * (size_t)w * h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            int t0[3], t1[3];                   /* vertical smoothing and vertical difference of the columns x - 1, x, x + 1 */
            for (int k = 0; k < 3; ++k) {
                const int xx = refl101(x + k - 1, w);
                const int s0 = L->img[(size_t)refl101(y - 1, h) * w + xx], s1 = L->img[(size_t)y * w + xx], s2 = L->img[(size_t)refl101(y + 1, h) * w + xx];
                t0[k] = (int16_t)((s0 + s2) * 3 + s1 * 10);
                t1[k] = (int16_t)(s2 - s0);
            }
            L->deriv[((size_t)y * w + x) * 2] = (int16_t)(t0[2] - t0[0]);
            L->deriv[((size_t)y * w + x) * 2 + 1] = (int16_t)((t1[2] + t1[0]) * 3 + t1[1] * 10);
        }
}

/* ---- the float sums ---------------------------------------------------------------------------------------------------------------- */
typedef struct { int order, win, overflow; double max_sum; } kr_sum;

static float note(kr_sum *S, float v) { if (fabs((double)v) > S->max_sum) S->max_sum = fabs((double)v); return v; }

static float tree21(kr_sum *S, float *v)
{
    for (int q = 0; q < 5; ++q) v[q] = note(S, v[q] + v[q + 16]);
    for (int q = 0; q < 8; ++q) v[q] = note(S, v[q] + v[q + 8]);
    for (int q = 0; q < 4; ++q) v[q] = note(S, v[q] + v[q + 4]);
    for (int q = 0; q < 2; ++q) v[q] = note(S, v[q] + v[q + 2]);
    return note(S, v[0] + v[1]);
}
static float tree64(kr_sum *S, float *v)
{
    float t[64];
    for (int l = 0; l < 64; ++l) t[l] = note(S, v[l] + v[l ^ 1]);
    for (int l = 0; l < 64; ++l) v[l] = note(S, t[l] + t[l ^ 2]);
    for (int l = 0; l < 64; ++l) t[l] = note(S, v[l] + v[(l & ~7) | (7 - (l & 7))]);
    for (int l = 0; l < 64; ++l) v[l] = note(S, t[l] + t[(l & ~15) | (15 - (l & 15))]);
    return note(S, note(S, note(S, v[0] + v[16]) + v[32]) + v[48]);
}
/* the owner of window pixel (x, y): lane index, or -1 for order 0 */
static int lane_of(const kr_sum *S, int x, int y)
{
    if (S->order == 1) return 3 * (y / 3) + x / 7;
    return 3 * y + x / 7;
}
/* sum of win * win integer terms (absval: of fabsf((float)term), the error) in the selected order; term[y * win + x] */
static float sum_terms(kr_sum *S, const int *term, int absval)
{
    const int win = S->win;
    if (S->order == 0) {
        float acc = 0.f;
        for (int i = 0; i < win * win; ++i) acc = note(S, acc + (absval ? fabsf((float)term[i]) : (float)term[i]));
        return acc;
    }
    float v[64];
    int32_t q32[64];
    int64_t q64[64];
    for (int l = 0; l < 64; ++l) { v[l] = 0.f; q32[l] = 0; q64[l] = 0; }
    for (int y = 0; y < win; ++y)                       /* rows outer, columns inner: the order inside a lane (matters for the error only) */
        for (int x = 0; x < win; ++x) {
            const int l = lane_of(S, x, y), t = term[y * win + x];
            if (absval) v[l] = note(S, v[l] + fabsf((float)t));
            else { q32[l] = (int32_t)((uint32_t)q32[l] + (uint32_t)t); q64[l] += t; }
        }
    if (!absval)
        for (int l = 0; l < 64; ++l) {
            if ((int64_t)q32[l] != q64[l]) S->overflow = 1;
            v[l] = note(S, (float)q32[l]);
        }
    return S->order == 1 ? tree21(S, v) : tree64(S, v);
}

static int cv_floor(float v) { return (int)floorf(v); }
static int cv_round_f(float v) { return (int)lrint((double)v); }
#define DESCALE(x, n) (((x) + (1 << ((n) - 1))) >> (n))
#define W_BITS 14

typedef struct { int iw00, iw01, iw10, iw11; } kr_w;
static kr_w weights(float a, float b)
{
    kr_w k;
    k.iw00 = cv_round_f((1.f - a) * (1.f - b) * (1 << W_BITS));
    k.iw01 = cv_round_f(a * (1.f - b) * (1 << W_BITS));
    k.iw10 = cv_round_f((1.f - a) * b * (1 << W_BITS));
    k.iw11 = (1 << W_BITS) - k.iw00 - k.iw01 - k.iw10;
    return k;
}
static int bil_I(const kr_level *L, int X, int Y, kr_w k)
{
    return DESCALE(I_at(L, X, Y) * k.iw00 + I_at(L, X + 1, Y) * k.iw01 + I_at(L, X, Y + 1) * k.iw10 + I_at(L, X + 1, Y + 1) * k.iw11, W_BITS - 5);
}
static int bil_D(const kr_level *L, int X, int Y, int c, kr_w k)
{
    return DESCALE(D_at(L, X, Y, c) * k.iw00 + D_at(L, X + 1, Y, c) * k.iw01 + D_at(L, X, Y + 1, c) * k.iw10 + D_at(L, X + 1, Y + 1, c) * k.iw11, W_BITS);
}

/* buildOpticalFlowPyramid's stop rule: the last level is the first whose successor would not exceed the window */
int kr_levels(int w, int h, int win, int max_level)
{
    int sw = w, sh = h;
    for (int level = 0; level <= max_level; ++level) {
        sw = (sw + 1) / 2; sh = (sh + 1) / 2;
        if (sw <= win || sh <= win) return level;
    }
    return max_level;
}

int kr_track(const uint8_t *const *prev_lv, const uint8_t *const *next_lv, const int *lw, const int *lh, int n_lv,
             const float *prev_pts, float *next_pts, int n, const kr_params *prm, int order,
             uint8_t *status, float *err, int32_t *exit_code, int32_t *iters, float *min_eig, double *max_sum)
{
    const int win = prm->win;
    /* the refusals of launch_klt_impl; the orders belong to their kernels */
    if (win < 3 || win > 21 || prm->max_level < 0 || prm->max_level >= KR_MAX_LEVELS || order < 0 || order > 2) return KR_E_INVALID;
    if ((order == 1 && win != 21) || (order == 2 && win > 20)) return KR_E_INVALID;
    const int max_level = kr_levels(lw[0], lh[0], win, prm->max_level);
    if (max_level + 1 > n_lv) return KR_E_LEVELS;
    const float FLT_SCALE = 1.f / (1 << 20);
    const int max_count = prm->max_iter < 0 ? 0 : prm->max_iter > 100 ? 100 : prm->max_iter;
    double epsilon = prm->eps < 0 ? 0 : prm->eps > 10 ? 10 : prm->eps;
    epsilon *= epsilon;
    const float min_eig_thr = (float)prm->min_eig_threshold;
    const float half = (win - 1) * 0.5f;
    kr_level pl[KR_MAX_LEVELS], nl[KR_MAX_LEVELS];
    for (int l = 0; l <= max_level; ++l) {
        pl[l].w = nl[l].w = lw[l]; pl[l].h = nl[l].h = lh[l];
        pl[l].img = prev_lv[l]; nl[l].img = next_lv[l]; nl[l].deriv = NULL;
        scharr(&pl[l]);
    }
    int *IWin = (int *)malloc(sizeof(int) * (size_t)win * win), *dIx = (int *)malloc(sizeof(int) * (size_t)win * win);
    int *dIy = (int *)malloc(sizeof(int) * (size_t)win * win), *term = (int *)malloc(sizeof(int) * (size_t)win * win);
    int *term2 = (int *)malloc(sizeof(int) * (size_t)win * win);
    int overflow = 0;
    for (int i = 0; i < n * KR_MAX_LEVELS; ++i) { exit_code[i] = KR_NOT_RUN; iters[i] = 0; min_eig[i] = 0.f; }

    /* points are independent: point outer, level inner (the kernels' loop nest; the oracle's is the other way round) */
    for (int p = 0; p < n; ++p) {
        kr_sum S = { order, win, 0, 0.0 };
        int st = 1;
        float ev = 0.f;
        float outx = prm->use_initial_flow ? next_pts[2 * p] : prev_pts[2 * p];
        float outy = prm->use_initial_flow ? next_pts[2 * p + 1] : prev_pts[2 * p + 1];
        for (int level = max_level; level >= 0; --level) {
            const kr_level *I = &pl[level], *J = &nl[level];
            int32_t *ex = &exit_code[p * KR_MAX_LEVELS + level], *it = &iters[p * KR_MAX_LEVELS + level];
            const float s = (float)(1. / (1 << level));
            float prevx = prev_pts[2 * p] * s, prevy = prev_pts[2 * p + 1] * s;
            float nx, ny;
            if (level == max_level) { nx = outx * s; ny = outy * s; }
            else { nx = outx * 2.f; ny = outy * 2.f; }
            outx = nx; outy = ny;
            prevx -= half; prevy -= half;
            const int ipx = cv_floor(prevx), ipy = cv_floor(prevy);
            if (ipx < -win || ipx >= I->w || ipy < -win || ipy >= I->h) {
                *ex = KR_REF_OUT;
                if (level == 0) { st = 0; ev = 0.f; }
                continue;
            }
            kr_w k = weights(prevx - ipx, prevy - ipy);
            for (int y = 0; y < win; ++y)
                for (int x = 0; x < win; ++x) {
                    IWin[y * win + x] = (int16_t)bil_I(I, ipx + x, ipy + y, k);
                    dIx[y * win + x] = (int16_t)bil_D(I, ipx + x, ipy + y, 0, k);
                    dIy[y * win + x] = (int16_t)bil_D(I, ipx + x, ipy + y, 1, k);
                }
            for (int i = 0; i < win * win; ++i) term[i] = dIx[i] * dIx[i];
            const float A11 = sum_terms(&S, term, 0) * FLT_SCALE;
            for (int i = 0; i < win * win; ++i) term[i] = dIx[i] * dIy[i];
            const float A12 = sum_terms(&S, term, 0) * FLT_SCALE;
            for (int i = 0; i < win * win; ++i) term[i] = dIy[i] * dIy[i];
            const float A22 = sum_terms(&S, term, 0) * FLT_SCALE;
            float D = A11 * A22 - A12 * A12;
            const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (2 * win * win);
            min_eig[p * KR_MAX_LEVELS + level] = minEig;
            if (minEig < min_eig_thr || D < FLT_EPSILON) {
                *ex = KR_EIG_FAIL;
                if (level == 0) st = 0;
                continue;
            }
            D = 1.f / D;
            nx -= half; ny -= half;
            float pdx = 0, pdy = 0;
            *ex = KR_MAX_ITER;
            for (int j = 0; j < max_count; ++j) {
                const int inx = cv_floor(nx), iny = cv_floor(ny);
                if (inx < -win || inx >= J->w || iny < -win || iny >= J->h) {
                    *ex = KR_GUESS_OUT; *it = j;
                    if (level == 0) st = 0;
                    break;
                }
                *it = j + 1;
                k = weights(nx - inx, ny - iny);
                for (int y = 0; y < win; ++y)
                    for (int x = 0; x < win; ++x) {
                        const int diff = bil_I(J, inx + x, iny + y, k) - IWin[y * win + x];
                        term[y * win + x] = diff * dIx[y * win + x];
                        term2[y * win + x] = diff * dIy[y * win + x];
                    }
                const float b1 = sum_terms(&S, term, 0) * FLT_SCALE, b2 = sum_terms(&S, term2, 0) * FLT_SCALE;
                const float dx = (float)((A12 * b2 - A22 * b1) * D), dy = (float)((A12 * b1 - A11 * b2) * D);
                nx += dx; ny += dy;
                outx = nx + half; outy = ny + half;
                if ((double)dx * dx + (double)dy * dy <= epsilon) { *ex = KR_CONVERGED; break; }
                if (j > 0 && fabsf(dx + pdx) < 0.01 && fabsf(dy + pdy) < 0.01) {
                    outx -= dx * 0.5f; outy -= dy * 0.5f;
                    *ex = KR_OSCILLATION;
                    break;
                }
                pdx = dx; pdy = dy;
            }
            if (st && level == 0) {
                const float qx = outx - half, qy = outy - half;
                const int inx = cv_floor(qx), iny = cv_floor(qy);
                if (inx < -win || inx >= J->w || iny < -win || iny >= J->h) { st = 0; *ex = KR_ERR_OUT; continue; }
                k = weights(qx - inx, qy - iny);
                for (int y = 0; y < win; ++y)
                    for (int x = 0; x < win; ++x) term[y * win + x] = bil_I(J, inx + x, iny + y, k) - IWin[y * win + x];
                ev = sum_terms(&S, term, 1) * 1.f / (32 * win * win);
            }
        }
        next_pts[2 * p] = outx; next_pts[2 * p + 1] = outy;
        status[p] = (uint8_t)st; err[p] = ev;
        max_sum[p] = S.max_sum;
        overflow |= S.overflow;
    }
    for (int l = 0; l <= max_level; ++l) free(pl[l].deriv);
    free(IWin); free(dIx); free(dIy); free(term); free(term2);
    return overflow ? KR_E_OVERFLOW : KR_OK;
}
