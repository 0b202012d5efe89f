/* Restatement of the stereo stage (ygz_slam_amd/csrc/stereo.hip): keypoint depths from a rectified pair, DESIGN.md section 19.  Plain C99, built
 * with gcc -O2 -ffp-contract=off -fno-fast-math; integer operations, + - * /, floor and ceil only.  The device is held to it bit for bit
 * (tests/test_gpu_stereo.py), and it is held to a numpy witness written another way (tests/test_stereo_ref.py).  Test infrastructure: never
 * part of the library. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SR_W 5          /* patch half-size */
#define SR_L 5          /* search half-range */
enum { SR_OK = 0, SR_NO_CANDIDATE, SR_DESCRIPTOR, SR_BORDER, SR_EDGE, SR_DISPARITY, SR_MEDIAN, SR_N_STATUS };

typedef struct { double baseline, min_disparity, max_disparity; int th_dist, write_depths; } sr_params;    /* = ygz_stereo_params */

int sr_params_size(void) { return (int)sizeof(sr_params); }

static int sr_hamming(const uint8_t *a, const uint8_t *b)
{
    int d = 0;
    for (int k = 0; k < 32; ++k) {
        unsigned x = (unsigned)(a[k] ^ b[k]);
        while (x) { d += (int)(x & 1u); x >>= 1; }
    }
    return d;
}

/* the per-pair rule: among the keypoints with status OK, med = element m / 2 of the ascending sads; 10 sad > 21 med -> MEDIAN (u_right and depth
 * back to -1); then the counts per status.  u_right, depth may be NULL. */
static int sr_cmp_i32(const void *a, const void *b) { const int32_t x = *(const int32_t *)a, y = *(const int32_t *)b; return (x > y) - (x < y); }
void sr_median_rule(int n, int32_t *status, const int32_t *sad, double *u_right, double *depth, int32_t *counts)
{
    int m = 0;
    int32_t *v = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) if (status[i] == SR_OK) v[m++] = sad[i];
    if (m > 0) {
        qsort(v, (size_t)m, sizeof(int32_t), sr_cmp_i32);
        const int64_t med = v[m / 2];
        for (int i = 0; i < n; ++i)
            if (status[i] == SR_OK && 10 * (int64_t)sad[i] > 21 * med) {
                status[i] = SR_MEDIAN;
                if (u_right) u_right[i] = -1.0;
                if (depth) depth[i] = -1.0;
            }
    }
    free(v);
    if (counts) {
        for (int k = 0; k < SR_N_STATUS; ++k) counts[k] = 0;
        for (int i = 0; i < n; ++i) counts[status[i]]++;
    }
}

/* left[l], right[l]: level l of the two pictures, lw[l] x lh[l], rows packed.  px [n][2] level-0 pixels, level [n], desc [n][32].
 * Outputs per left keypoint (any may be NULL): right_idx, u_right, depth, sad, status as the ABI; best_idx, best_dist, n_cand, sads [nL][11] as
 * ygz_hip_stereo_candidates; delta [nL] the parabola's offset (0 where step 8 was not reached), k_out [nL] the SAD minimum's inc (-99 likewise). */
void sr_match(int n_levels, const int32_t *lw, const int32_t *lh, const uint8_t *const *left, const uint8_t *const *right, double fx_d,
              const double *pxL, const int32_t *levelL, const uint8_t *descL, int nL,
              const double *pxR, const int32_t *levelR, const uint8_t *descR, int nR, const sr_params *p,
              int32_t *right_idx, double *u_right, double *depth, int32_t *sad, int32_t *status, int32_t *counts,
              int32_t *best_idx, int32_t *best_dist, int32_t *n_cand, int32_t *sads, double *delta, int32_t *k_out)
{
    const double bf = fx_d * p->baseline, minD = p->min_disparity, maxD = p->max_disparity == 0.0 ? fx_d : p->max_disparity;
    int32_t *st = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nL > 0 ? nL : 1)), *sd = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nL > 0 ? nL : 1));
    double *ur = (double *)malloc(sizeof(double) * (size_t)(nL > 0 ? nL : 1)), *dp = (double *)malloc(sizeof(double) * (size_t)(nL > 0 ? nL : 1));
    (void)n_levels;
    for (int i = 0; i < nL; ++i) {
        const double uL = pxL[2 * i], vL = pxL[2 * i + 1];
        const int l = levelL[i];
        int bj = -1, bd = 1 << 20, nc = 0, D[2 * SR_L + 1], reached = 0, k = -99;
        double dl = 0.0;
        st[i] = SR_NO_CANDIDATE; sd[i] = -1; ur[i] = -1.0; dp[i] = -1.0;
        if (right_idx) right_idx[i] = -1;
        do {
            if (uL - minD < 0.0) break;                                                       /* 1 */
            const double lo = uL - maxD, hi = uL - minD, fvL = floor(vL);
            for (int j = 0; j < nR; ++j) {                                                    /* 2, 3 */
                const int lr = levelR[j];
                const double uR = pxR[2 * j], vR = pxR[2 * j + 1];
                if (lr - l > 1 || l - lr > 1) continue;
                const double r = 2.0 * (double)(1 << lr);
                if (!(floor(vR - r) <= fvL && fvL <= ceil(vR + r))) continue;
                if (!(uR >= lo && uR <= hi)) continue;
                ++nc;
                const int d = sr_hamming(descL + 32 * (size_t)i, descR + 32 * (size_t)j);
                if (d < bd) { bd = d; bj = j; }
            }
            if (bj < 0) break;
            if (bd >= p->th_dist) { st[i] = SR_DESCRIPTOR; break; }
            const double s = (double)(1 << l);                                                /* 4 */
            const int su = (int)floor(uL / s + 0.5), sv = (int)floor(vL / s + 0.5), sr = (int)floor(pxR[2 * bj] / s + 0.5);
            const int Wl = lw[l], Hl = lh[l];
            if (!(SR_W <= su && su < Wl - SR_W && SR_W <= sv && sv < Hl - SR_W && sr - SR_L - SR_W >= 0 && sr + SR_L + SR_W < Wl)) {   /* 5 */
                st[i] = SR_BORDER; break;
            }
            const uint8_t *IL = left[l], *IR = right[l];
            const int cL = IL[(size_t)sv * Wl + su];
            int best = 1 << 30;
            for (int inc = -SR_L; inc <= SR_L; ++inc) {                                       /* 6 */
                const int cR = IR[(size_t)sv * Wl + sr + inc];
                int acc = 0;
                for (int dy = -SR_W; dy <= SR_W; ++dy)
                    for (int dx = -SR_W; dx <= SR_W; ++dx) {
                        const int a = (int)IL[(size_t)(sv + dy) * Wl + su + dx] - cL, b = (int)IR[(size_t)(sv + dy) * Wl + sr + inc + dx] - cR;
                        acc += a > b ? a - b : b - a;
                    }
                D[inc + SR_L] = acc;
                if (acc < best) { best = acc; k = inc; }
            }
            reached = 1;
            if (k == -SR_L || k == SR_L) { st[i] = SR_EDGE; break; }                          /* 7 */
            const int d1 = D[k - 1 + SR_L], d2 = D[k + SR_L], d3 = D[k + 1 + SR_L];          /* 8 */
            const int den = d1 + d3 - 2 * d2;
            dl = (double)(d1 - d3) / (double)(2 * den);
            double uRs = s * ((double)(sr + k) + dl);
            double disp = uL - uRs;
            if (!(disp >= minD && disp < maxD)) { st[i] = SR_DISPARITY; break; }             /* 9 */
            if (disp <= 0.0) { disp = 0.01; uRs = uL - 0.01; }
            st[i] = SR_OK; ur[i] = uRs; dp[i] = bf / disp; sd[i] = d2;                        /* 10 */
            if (right_idx) right_idx[i] = bj;
        } while (0);
        if (best_idx) best_idx[i] = bj;
        if (best_dist) best_dist[i] = bj < 0 ? -1 : bd;
        if (n_cand) n_cand[i] = nc;
        if (sads) for (int q = 0; q < 2 * SR_L + 1; ++q) sads[(2 * SR_L + 1) * (size_t)i + q] = reached ? D[q] : -1;
        if (delta) delta[i] = dl;
        if (k_out) k_out[i] = reached ? k : -99;
    }
    sr_median_rule(nL, st, sd, ur, dp, counts);
    for (int i = 0; i < nL; ++i) {
        if (status) status[i] = st[i];
        if (sad) sad[i] = sd[i];
        if (u_right) u_right[i] = ur[i];
        if (depth) depth[i] = dp[i];
    }
    free(st); free(sd); free(ur); free(dp);
}
