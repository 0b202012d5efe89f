/* lfuse_ref.c -- the frozen restatement of the local-map fusion search (ygz_slam_amd/csrc/lfuse.hip): the search of
 * ORB-SLAM2's ORBmatcher::Fuse(pKF, vpMapPoints, th) as LocalMapping::SearchInNeighbors uses it, for many target keyframes that read shared
 * point sets.  Test infrastructure: built with gcc -O2 -ffp-contract=off -fno-fast-math, double arithmetic with + - * / sqrt only.
 *
 * Steps 1-6 of a (problem, point) are pr_project of proj_ref.c, included unchanged, with S = (q, t, 1): skip flag, z > 0, image bounds,
 * distance range, viewing angle, predicted level.  Step 6b: ur = u - bf iz with bf = fx baseline formed once per call and iz = 1 / z, z in
 * pr_project's operation order.  Step 7: the window r = th 2^pred over the keypoints of levels pred-1 .. pred that are not taken.  Step 7b,
 * the gate: ex = u - kx, ey = v - ky, e2 = ex ex + ey ey; a mono keypoint (kp_ur NULL or kp_ur[j] < 0) is rejected when e2 > chi2_mono
 * 4^level, a stereo keypoint with er = ur - kp_ur[j], e2 = e2 + er er when e2 > chi2_stereo 4^level; n_gated counts the keypoints in the
 * window that the gate rejected.  Step 8: the smallest (Hamming distance, keypoint index) of the survivors, a match when its distance is
 * <= th_dist, else match = dist = -1.  No claim, no list. */
#include <stddef.h>
#include "proj_ref.c"

typedef struct {                         /* the layout of ygz_lfuse_points (include/ygz_hip.h) */
    const double  *pw;
    const uint8_t *pt_desc;
    const double  *pt_dmax;
    const double  *pt_normal;
    int            n_pt;
} lf_points;

typedef struct {                         /* the layout of ygz_lfuse_problem */
    double         T[7];
    const double  *kp_px;
    const int32_t *kp_level;
    const uint8_t *kp_desc;
    const double  *kp_ur;
    const uint8_t *kp_taken;
    const uint8_t *pt_skip;
    int            n_kp;
    int            set;
} lf_problem;

typedef struct { double th, baseline, chi2_mono, chi2_stereo; int32_t th_dist, pad; } lf_params;

size_t lf_points_size(void) { return sizeof(lf_points); }
size_t lf_problem_size(void) { return sizeof(lf_problem); }
size_t lf_params_size(void) { return sizeof(lf_params); }
size_t lf_offset(int which, int k)
{
    static const size_t pt[] = { offsetof(lf_points, pw), offsetof(lf_points, pt_desc), offsetof(lf_points, pt_dmax), offsetof(lf_points, pt_normal),
                                 offsetof(lf_points, n_pt) };
    static const size_t pb[] = { offsetof(lf_problem, T), offsetof(lf_problem, kp_px), offsetof(lf_problem, kp_level), offsetof(lf_problem, kp_desc),
                                 offsetof(lf_problem, kp_ur), offsetof(lf_problem, kp_taken), offsetof(lf_problem, pt_skip), offsetof(lf_problem, n_kp),
                                 offsetof(lf_problem, set) };
    static const size_t pr[] = { offsetof(lf_params, th), offsetof(lf_params, baseline), offsetof(lf_params, chi2_mono),
                                 offsetof(lf_params, chi2_stereo), offsetof(lf_params, th_dist), offsetof(lf_params, pad) };
    return which == 0 ? pt[k] : (which == 1 ? pb[k] : pr[k]);
}

void lf_default_params(lf_params *p)
{
    p->th = 3.0; p->baseline = 0.1; p->chi2_mono = 5.99; p->chi2_stereo = 7.8; p->th_dist = 50; p->pad = 0;
}

/* one problem: every output [n_pt of its set]; each may be NULL.  counts [2] = matches, points searched */
static void lf_problem_search(const lf_points *S, const lf_problem *B, const double K4[4], int w, int h, int L, const lf_params *prm, double bf,
                              int32_t *match, int32_t *dist, int32_t *pred_level, int32_t *reason, int32_t *n_gated, int32_t *counts)
{
    pr_problem P;
    memset(&P, 0, sizeof P);
    P.pw = S->pw; P.pt_desc = S->pt_desc; P.pt_dmax = S->pt_dmax; P.pt_normal = S->pt_normal; P.pt_skip = B->pt_skip; P.n_pt = S->n_pt;
    for (int k = 0; k < 7; ++k) P.S[k] = B->T[k];
    P.S[7] = 1.0;
    double R[9];
    pr_rotation(P.S, R);
    int nm = 0, ns = 0;
    for (int i = 0; i < S->n_pt; ++i) {
        double u, v;
        int pred;
        const int why = pr_project(&P, K4, w, h, L, i, &u, &v, &pred);
        int m = -1, dd = -1, ng = 0;
        if (why == PR_KEPT) {
            const double *X = S->pw + 3 * (size_t)i;
            const double z = 1.0 * (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + P.S[6];         /* pr_project's z */
            const double iz = 1 / z;
            const double ur = u - bf * iz;
            const double r = prm->th * (double)(1 << pred);
            ++ns;
            for (int j = 0; j < B->n_kp; ++j) {
                if (B->kp_taken && B->kp_taken[j]) continue;
                const int lv = B->kp_level[j];
                if (lv < pred - 1 || lv > pred) continue;
                const double kx = B->kp_px[2 * (size_t)j], ky = B->kp_px[2 * (size_t)j + 1];
                const double dx = kx - u, dy = ky - v;
                if (!(dx < r && dx > -r && dy < r && dy > -r)) continue;
                const double ex = u - kx, ey = v - ky, s2 = (double)(1 << (2 * lv));
                double e2 = ex * ex + ey * ey;
                const double kur = B->kp_ur ? B->kp_ur[j] : -1.0;
                if (kur >= 0) {
                    const double er = ur - kur;
                    e2 = e2 + er * er;
                    if (e2 > prm->chi2_stereo * s2) { ++ng; continue; }
                } else if (e2 > prm->chi2_mono * s2) { ++ng; continue; }
                const int d = pr_hamming(S->pt_desc + 32 * (size_t)i, B->kp_desc + 32 * (size_t)j);
                if (m < 0 || d < dd) { m = j; dd = d; }                                         /* j grows: a tie stays with the smaller */
            }
            if (m >= 0 && dd > prm->th_dist) { m = -1; dd = -1; }
            if (m >= 0) ++nm;
        }
        if (match) match[i] = m;
        if (dist) dist[i] = dd;
        if (pred_level) pred_level[i] = pred;
        if (reason) reason[i] = why;
        if (n_gated) n_gated[i] = ng;
    }
    if (counts) { counts[0] = nm; counts[1] = ns; }
}

/* the call: outputs concatenated in problem order, each problem n_pt entries of its set; any output may be NULL */
void lf_search(int n_sets, const lf_points *sets, int n_problems, const lf_problem *problems, const double K4[4], int w, int h, int L,
               const lf_params *prm, int32_t *match, int32_t *dist, int32_t *pred_level, int32_t *reason, int32_t *n_gated, int32_t *counts)
{
    const double bf = K4[0] * prm->baseline;
    size_t off = 0;
    (void)n_sets;
    for (int q = 0; q < n_problems; ++q) {
        const lf_points *S = sets + problems[q].set;
        lf_problem_search(S, problems + q, K4, w, h, L, prm, bf, match ? match + off : NULL, dist ? dist + off : NULL,
                          pred_level ? pred_level + off : NULL, reason ? reason + off : NULL, n_gated ? n_gated + off : NULL,
                          counts ? counts + 2 * q : NULL);
        off += (size_t)S->n_pt;
    }
}
