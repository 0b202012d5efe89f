/* The restatement of the local-map selection (ygz_slam_amd/csrc/lms.hip, include/ygz_hip.h): the keyframe votes of a
 * frame's map points, StereoTracker::LocalKeyFrames' list (the voters in index order, then one covisible keyframe per voter) and the local
 * point set in (rank of the first local observer, its feature index, point) order with the frame's `prior` row, for many frames on one map.
 * Written the plain way -- per frame a walk over its entries, per point a walk over its list, the set by qsort.  Every output is an integer:
 * the device call has to equal it bit for bit.  Test infrastructure (gcc -O2), never linked into the package. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    int32_t max_keyframes, max_points;
} lr_params;

typedef struct {
    int32_t rank, feat, point;
} lr_key;

static int by_key(const void *a, const void *b)
{
    const lr_key *x = (const lr_key *)a, *y = (const lr_key *)b;
    if (x->rank != y->rank) return x->rank < y->rank ? -1 : 1;
    if (x->feat != y->feat) return x->feat < y->feat ? -1 : 1;
    return x->point < y->point ? -1 : (x->point > y->point ? 1 : 0);
}

/* votes, local_kf [F][K]; ref, n_voters, n_local, n_pt, n_cut [F]; local_pt [F][max_points]; fr_prior [fr_off[F]].  pt_bad may be NULL.
 * Returns 0, or -1 when memory runs out */
int lr_select(int K, const uint8_t *kf_bad, int C, const int32_t *cov, int n_points, const int32_t *offsets, const int32_t *kf,
              const int32_t *feat, const uint8_t *pt_bad, int n_frames, const int32_t *fr_off, const int32_t *fr_pt, const lr_params *q,
              int32_t *votes, int32_t *ref, int32_t *n_voters, int32_t *n_local, int32_t *local_kf, int32_t *n_pt, int32_t *n_cut,
              int32_t *local_pt, int32_t *fr_prior)
{
    int32_t *rank = (int32_t *)malloc((size_t)K * sizeof(int32_t));
    int32_t *pos = (int32_t *)malloc((size_t)n_points * sizeof(int32_t));
    lr_key *keys = (lr_key *)malloc((size_t)n_points * sizeof(lr_key));
    if (!rank || !pos || !keys) { free(rank); free(pos); free(keys); return -1; }
    for (int f = 0; f < n_frames; ++f) {
        int32_t *v = votes + (size_t)f * K, *list = local_kf + (size_t)f * K, *set = local_pt + (size_t)f * q->max_points;
        /* 1 */
        memset(v, 0, (size_t)K * sizeof(int32_t));
        for (int e = fr_off[f]; e < fr_off[f + 1]; ++e) {
            const int p = fr_pt[e];
            if (p < 0 || (pt_bad && pt_bad[p])) continue;
            for (int g = offsets[p]; g < offsets[p + 1]; ++g) ++v[kf[g]];
        }
        /* 2 */
        int best = -1;
        for (int k = 0; k < K; ++k)
            if (v[k] > 0 && (best < 0 || v[k] > v[best])) best = k;
        ref[f] = best;
        /* 3 */
        int n = 0;
        for (int k = 0; k < K; ++k) { rank[k] = -1; list[k] = -1; }
        for (int k = 0; k < K; ++k)
            if (v[k] > 0 && !kf_bad[k]) { rank[k] = n; list[n++] = k; }
        const int voters = n;
        n_voters[f] = voters;
        for (int i = 0; i < voters && n < q->max_keyframes; ++i) {
            const int32_t *row = cov + (size_t)list[i] * C;
            for (int j = 0; j < C; ++j) {
                const int c = row[j];
                if (c < 0 || kf_bad[c] || rank[c] >= 0) continue;
                rank[c] = n; list[n++] = c;
                break;
            }
        }
        n_local[f] = n;
        /* 4 */
        int m = 0;
        for (int p = 0; p < n_points; ++p) {
            pos[p] = -1;
            if (pt_bad && pt_bad[p]) continue;
            int at = -1;
            for (int g = offsets[p]; g < offsets[p + 1]; ++g)
                if (rank[kf[g]] >= 0 && (at < 0 || rank[kf[g]] < rank[kf[at]])) at = g;
            if (at < 0) continue;
            keys[m].rank = rank[kf[at]]; keys[m].feat = feat[at]; keys[m].point = p;
            ++m;
        }
        qsort(keys, (size_t)m, sizeof(lr_key), by_key);
        const int kept = m < q->max_points ? m : q->max_points;
        for (int i = 0; i < q->max_points; ++i) set[i] = i < kept ? keys[i].point : -1;
        for (int i = 0; i < kept; ++i) pos[keys[i].point] = i;
        n_pt[f] = kept;
        n_cut[f] = m - kept;
        /* 5 */
        for (int e = fr_off[f]; e < fr_off[f + 1]; ++e) fr_prior[e] = fr_pt[e] < 0 ? -1 : pos[fr_pt[e]];
    }
    free(rank); free(pos); free(keys);
    return 0;
}
