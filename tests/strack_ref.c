/* strack_ref.c -- the frozen restatement of the stereo tracking search (ygz_slam_amd/csrc/strack.hip): ORB-SLAM2's
 * ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (mode 0, FRAME) and SearchByProjection(F, vpMapPoints, th) (mode 1,
 * LOCAL) on one primitive, with the right-column gate.  Test infrastructure: built with gcc -O2 -ffp-contract=off -fno-fast-math, double
 * arithmetic with + - * / sqrt only, every expression in the order the kernel uses.
 *
 * Device part, per (problem, point); the first failing step sets the reason (0 searched, 1 skip, 2 behind, 3 outside, 4 range, 5 angle):
 *   1-2  pr_project of proj_ref.c, included unchanged, with S = (q, t, 1): skip flag, z > 0, u, v inside [0, w) x [0, h); iz = 1 / z and
 *        ur = u - bf iz, bf = fx baseline formed once per call.  A FRAME point has no distance range: pr_project is given the point's own
 *        distance as dmax, which its range test always accepts.
 *   3    FRAME: lvl = pt_level[i], r = th 2^lvl, levels [lvl-1, lvl+1] (direction 0), [lvl, L-1] (+1), [0, lvl] (-1); level = lvl.
 *   4    LOCAL: pr_project's distance range, viewing angle and predicted level; f = r_near when Xc.(R n) > cos_near d, else r_wide;
 *        r = (th f) 2^pred, levels [pred-1, pred]; level = pred.
 *   5    candidates: keypoints that are not taken, of a level in the range, with |kx - u| < r and |ky - v| < r (open).
 *   6    the right-column gate: a stereo candidate (kp_ur[j] >= 0) with |ur - kp_ur[j]| > r is rejected (n_gated); n_cand the survivors.
 *   7    the survivors sorted by (Hamming distance, keypoint index), cut to the first ST_TOPK; no distance threshold.
 * Host part, per problem, points in index order:
 *   8    the claim walk: e1, e2 the first two entries of the list that are not taken; none -> outcome 1; dist(e1) > th_dist -> 2; LOCAL with
 *        e2 of e1's level and (double)dist(e1) > ratio (double)dist(e2) -> 3; else outcome 0: match = e1, taken[e1] = 1.  reason != 0: -1.
 *   9    FRAME with pt_angle and check_orientation: rot = (float)(pt_angle[i] - kp_angle[match]), + 360 when negative, bin = round(rot
 *        (1.0f / 30)), 30 -> 0; the histogram over 30 bins and its three maxima; a match of another bin (or of none) loses match and dist
 *        (outcome 4) and keeps its keypoint claimed. */
#include <stddef.h>
#include "proj_ref.c"

#define ST_TOPK 8
#define ST_MAX_PROBLEMS 64
#define ST_MAX_SETS 8
#define ST_MAX_PAIRS 262144

typedef struct {                         /* the layout of ygz_strack_points (include/ygz_hip.h) */
    const double  *pw;
    const uint8_t *pt_desc;
    const int32_t *pt_level;
    const double  *pt_angle;
    const double  *pt_dmax;
    const double  *pt_normal;
    int            n_pt;
} st_points;

typedef struct {                         /* the layout of ygz_strack_problem */
    double         T[7];
    double         th;
    const double  *kp_px;
    const int32_t *kp_level;
    const uint8_t *kp_desc;
    const double  *kp_ur;
    const double  *kp_angle;
    const uint8_t *kp_taken;
    const uint8_t *pt_skip;
    int            n_kp;
    int            set;
    int            mode;
    int            direction;
} st_problem;

typedef struct { double baseline, ratio, r_near, r_wide, cos_near; int32_t th_dist, check_orientation; } st_params;

size_t st_points_size(void) { return sizeof(st_points); }
size_t st_problem_size(void) { return sizeof(st_problem); }
size_t st_params_size(void) { return sizeof(st_params); }
int st_limit(int k) { static const int v[] = { ST_MAX_PROBLEMS, ST_MAX_SETS, ST_MAX_PAIRS, ST_TOPK }; return v[k]; }
size_t st_offset(int which, int k)
{
    static const size_t pt[] = { offsetof(st_points, pw), offsetof(st_points, pt_desc), offsetof(st_points, pt_level), offsetof(st_points, pt_angle),
                                 offsetof(st_points, pt_dmax), offsetof(st_points, pt_normal), offsetof(st_points, n_pt) };
    static const size_t pb[] = { offsetof(st_problem, T), offsetof(st_problem, th), offsetof(st_problem, kp_px), offsetof(st_problem, kp_level),
                                 offsetof(st_problem, kp_desc), offsetof(st_problem, kp_ur), offsetof(st_problem, kp_angle),
                                 offsetof(st_problem, kp_taken), offsetof(st_problem, pt_skip), offsetof(st_problem, n_kp), offsetof(st_problem, set),
                                 offsetof(st_problem, mode), offsetof(st_problem, direction) };
    static const size_t pr[] = { offsetof(st_params, baseline), offsetof(st_params, ratio), offsetof(st_params, r_near), offsetof(st_params, r_wide),
                                 offsetof(st_params, cos_near), offsetof(st_params, th_dist), offsetof(st_params, check_orientation) };
    return which == 0 ? pt[k] : (which == 1 ? pb[k] : pr[k]);
}

void st_default_params(st_params *p)
{
    p->baseline = 0.1; p->ratio = 0.8; p->r_near = 2.5; p->r_wide = 4.0; p->cos_near = 0.998; p->th_dist = 100; p->check_orientation = 1;
}

/* steps 1-7 of one (problem, point): the reason; u, v, ur, level, r and the level range for reason 0 */
static int st_point(const st_points *S, const st_problem *B, const double K4[4], int w, int h, int L, const st_params *prm, double bf, int i,
                    double uvr[3], int *level, double *r_out, int *lo_out, int *hi_out)
{
    pr_problem P;
    double R[9], u, v, dm = 0;
    int pred;
    memset(&P, 0, sizeof P);
    for (int k = 0; k < 7; ++k) P.S[k] = B->T[k];
    P.S[7] = 1.0;
    pr_rotation(P.S, R);
    const double *X = S->pw + 3 * (size_t)i;
    const double x = 1.0 * (R[0] * X[0] + R[1] * X[1] + R[2] * X[2]) + P.S[4];            /* pr_project's x, y, z */
    const double y = 1.0 * (R[3] * X[0] + R[4] * X[1] + R[5] * X[2]) + P.S[5];
    const double z = 1.0 * (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + P.S[6];
    const double d = sqrt(x * x + y * y + z * z);
    P.pw = X; P.pt_skip = B->pt_skip ? B->pt_skip + i : NULL; P.n_pt = 1;
    if (B->mode == 0) { dm = d; P.pt_dmax = &dm; P.pt_normal = NULL; }
    else { P.pt_dmax = S->pt_dmax + i; P.pt_normal = S->pt_normal + 3 * (size_t)i; }
    uvr[0] = uvr[1] = uvr[2] = 0;
    *level = -1; *r_out = 0; *lo_out = 0; *hi_out = -1;
    const int why = pr_project(&P, K4, w, h, L, 0, &u, &v, &pred);
    if (why != PR_KEPT) return why;
    const double iz = 1 / z;
    uvr[0] = u; uvr[1] = v; uvr[2] = u - bf * iz;
    if (B->mode == 0) {
        const int lvl = S->pt_level[i];
        *level = lvl;
        *r_out = B->th * (double)(1 << lvl);
        if (B->direction > 0) { *lo_out = lvl; *hi_out = L - 1; }
        else if (B->direction < 0) { *lo_out = 0; *hi_out = lvl; }
        else { *lo_out = lvl - 1; *hi_out = lvl + 1; }
    } else {
        const double *n = S->pt_normal + 3 * (size_t)i;
        const double nx = R[0] * n[0] + R[1] * n[1] + R[2] * n[2];
        const double ny = R[3] * n[0] + R[4] * n[1] + R[5] * n[2];
        const double nz = R[6] * n[0] + R[7] * n[1] + R[8] * n[2];
        const double f = (x * nx + y * ny + z * nz > prm->cos_near * d) ? prm->r_near : prm->r_wide;
        *level = pred;
        *r_out = (B->th * f) * (double)(1 << pred);
        *lo_out = pred - 1; *hi_out = pred;
    }
    return PR_KEPT;
}

/* one problem: every output [n_pt of its set] (proj [n_pt][3], cand [n_pt][ST_TOPK]); each may be NULL.  counts [4], rot [33] */
static void st_problem_search(const st_points *S, const st_problem *B, const double K4[4], int w, int h, int L, const st_params *prm, double bf,
                              int32_t *match, int32_t *dist, int32_t *level, int32_t *reason, int32_t *outcome, int32_t *n_cand,
                              int32_t *n_gated, double *proj, int32_t *cand, int32_t *counts, int32_t *rot)
{
    const int n = S->n_pt;
    int32_t *ci = (int32_t *)malloc((size_t)(n + 1) * ST_TOPK * 4), *cd = (int32_t *)malloc((size_t)(n + 1) * ST_TOPK * 4);
    int32_t *nc = (int32_t *)malloc((size_t)(n + 1) * 4), *why_ = (int32_t *)malloc((size_t)(n + 1) * 4);
    int32_t *m_ = (int32_t *)malloc((size_t)(n + 1) * 4), *d_ = (int32_t *)malloc((size_t)(n + 1) * 4), *oc = (int32_t *)malloc((size_t)(n + 1) * 4);
    uint8_t *taken = (uint8_t *)calloc((size_t)B->n_kp, 1);
    int nm = 0, ns = 0, nov = 0, nrot = 0;
    for (int i = 0; i < n; ++i) {
        double uvr[3], r;
        int lvl, lo, hi, ng = 0, cnt = 0;
        const int why = st_point(S, B, K4, w, h, L, prm, bf, i, uvr, &lvl, &r, &lo, &hi);
        int32_t *li = ci + (size_t)ST_TOPK * i, *ld = cd + (size_t)ST_TOPK * i;
        for (int k = 0; k < ST_TOPK; ++k) { li[k] = -1; ld[k] = -1; }
        if (why == PR_KEPT) {
            const double u = uvr[0], v = uvr[1], ur = uvr[2];
            ++ns;
            for (int j = 0; j < B->n_kp; ++j) {
                if (B->kp_taken && B->kp_taken[j]) continue;
                const int lv = B->kp_level[j];
                if (lv < lo || lv > hi) continue;
                const double dx = B->kp_px[2 * (size_t)j] - u, dy = B->kp_px[2 * (size_t)j + 1] - v;
                if (!(dx < r && dx > -r && dy < r && dy > -r)) continue;
                const double kur = B->kp_ur ? B->kp_ur[j] : -1.0;
                if (kur >= 0) {
                    const double er = ur - kur;
                    if (er > r || er < -r) { ++ng; continue; }
                }
                const int dd = pr_hamming(S->pt_desc + 32 * (size_t)i, B->kp_desc + 32 * (size_t)j);
                ++cnt;
                /* insertion by (distance, index): j grows, so an equal distance goes behind */
                int k = cnt - 1 < ST_TOPK ? cnt - 1 : ST_TOPK;
                while (k > 0 && ld[k - 1] > dd) --k;
                if (k >= ST_TOPK) continue;
                const int last = cnt - 1 < ST_TOPK - 1 ? cnt - 1 : ST_TOPK - 1;
                for (int m = last; m > k; --m) { li[m] = li[m - 1]; ld[m] = ld[m - 1]; }
                li[k] = j; ld[k] = dd;
            }
            if (cnt > ST_TOPK) ++nov;
        }
        nc[i] = cnt; why_[i] = why;
        if (level) level[i] = lvl;
        if (reason) reason[i] = why;
        if (n_cand) n_cand[i] = cnt;
        if (n_gated) n_gated[i] = ng;
        if (proj) { proj[3 * (size_t)i] = uvr[0]; proj[3 * (size_t)i + 1] = uvr[1]; proj[3 * (size_t)i + 2] = uvr[2]; }
    }
    if (cand) memcpy(cand, ci, (size_t)n * ST_TOPK * 4);
    /* step 8 */
    if (B->kp_taken) memcpy(taken, B->kp_taken, (size_t)B->n_kp);
    for (int i = 0; i < n; ++i) {
        m_[i] = -1; d_[i] = -1; oc[i] = -1;
        if (why_[i] != PR_KEPT) continue;
        const int len = nc[i] < ST_TOPK ? nc[i] : ST_TOPK;
        int e1 = -1, e2 = -1;
        for (int k = 0; k < len; ++k) {
            if (taken[ci[(size_t)ST_TOPK * i + k]]) continue;
            if (e1 < 0) e1 = k; else { e2 = k; break; }
        }
        if (e1 < 0) { oc[i] = 1; continue; }
        const int j1 = ci[(size_t)ST_TOPK * i + e1], d1 = cd[(size_t)ST_TOPK * i + e1];
        if (d1 > prm->th_dist) { oc[i] = 2; continue; }
        if (B->mode == 1 && e2 >= 0) {
            const int j2 = ci[(size_t)ST_TOPK * i + e2], d2 = cd[(size_t)ST_TOPK * i + e2];
            if (B->kp_level[j1] == B->kp_level[j2] && (double)d1 > prm->ratio * (double)d2) { oc[i] = 3; continue; }
        }
        oc[i] = 0; m_[i] = j1; d_[i] = d1; taken[j1] = 1;
    }
    /* step 9 */
    int32_t hist[30], ind[3] = { -1, -1, -1 };
    for (int b = 0; b < 30; ++b) hist[b] = 0;
    if (B->mode == 0 && S->pt_angle && prm->check_orientation) {
        const float factor = 1.0f / 30;
        int32_t *bin_ = why_;                                       /* reused: the bin of every match */
        for (int i = 0; i < n; ++i) {
            bin_[i] = -1;
            if (m_[i] < 0) continue;
            float rot_ = (float)(S->pt_angle[i] - B->kp_angle[m_[i]]);
            if (rot_ < 0) rot_ += 360;
            const float fb = rot_ * factor;
            int bin = (int)((double)fb + 0.5);                      /* round of a value >= 0 */
            if (bin == 30) bin = 0;
            if (!(fb >= 0) || bin < 0 || bin >= 30) continue;
            bin_[i] = bin;
            hist[bin]++;
        }
        int max1 = 0, max2 = 0, max3 = 0;
        for (int b = 0; b < 30; ++b) {
            const int s = hist[b];
            if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind[2] = ind[1]; ind[1] = ind[0]; ind[0] = b; }
            else if (s > max2) { max3 = max2; max2 = s; ind[2] = ind[1]; ind[1] = b; }
            else if (s > max3) { max3 = s; ind[2] = b; }
        }
        if ((float)max2 < 0.1f * (float)max1) { ind[1] = -1; ind[2] = -1; }
        else if ((float)max3 < 0.1f * (float)max1) { ind[2] = -1; }
        for (int i = 0; i < n; ++i) {
            if (m_[i] < 0) continue;
            if (bin_[i] >= 0 && (bin_[i] == ind[0] || bin_[i] == ind[1] || bin_[i] == ind[2])) continue;
            m_[i] = -1; d_[i] = -1; oc[i] = 4; ++nrot;
        }
    }
    for (int i = 0; i < n; ++i) if (m_[i] >= 0) ++nm;
    if (match) memcpy(match, m_, (size_t)n * 4);
    if (dist) memcpy(dist, d_, (size_t)n * 4);
    if (outcome) memcpy(outcome, oc, (size_t)n * 4);
    if (counts) { counts[0] = nm; counts[1] = ns; counts[2] = nov; counts[3] = nrot; }
    if (rot) { for (int b = 0; b < 30; ++b) rot[b] = hist[b]; rot[30] = ind[0]; rot[31] = ind[1]; rot[32] = ind[2]; }
    free(ci); free(cd); free(nc); free(why_); free(m_); free(d_); free(oc); free(taken);
}

/* the call: outputs concatenated in problem order, each problem n_pt entries of its set; any output may be NULL */
void st_search(int n_sets, const st_points *sets, int n_problems, const st_problem *problems, const double K4[4], int w, int h, int L,
               const st_params *prm, int32_t *match, int32_t *dist, int32_t *level, int32_t *reason, int32_t *outcome, int32_t *n_cand,
               int32_t *n_gated, double *proj, int32_t *cand, int32_t *counts, int32_t *rot)
{
    const double bf = K4[0] * prm->baseline;
    size_t off = 0;
    (void)n_sets;
    for (int q = 0; q < n_problems; ++q) {
        const st_points *S = sets + problems[q].set;
        st_problem_search(S, problems + q, K4, w, h, L, prm, bf, match ? match + off : NULL, dist ? dist + off : NULL, level ? level + off : NULL,
                          reason ? reason + off : NULL, outcome ? outcome + off : NULL, n_cand ? n_cand + off : NULL,
                          n_gated ? n_gated + off : NULL, proj ? proj + 3 * off : NULL, cand ? cand + ST_TOPK * off : NULL,
                          counts ? counts + 4 * q : NULL, rot ? rot + 33 * q : NULL);
        off += (size_t)S->n_pt;
    }
}
