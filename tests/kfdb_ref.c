/* Restatement of the keyframe database's query (ygz_slam_amd/csrc/kfdb.hip) in plain C: per (query, entry) a two-pointer
 * merge over the two ascending word lists.  common counts the shared words; score = -s / 2 with s = 0.0 and, per shared word in ascending
 * order, s += fabs(v - w) - fabs(v) - fabs(w) (v the query's weight, w the row's): DBoW3::L1Scoring::score.  A dead row (n < 0) gives -1 and 0.
 * gcc -std=c99 -O2 -ffp-contract=off -fno-fast-math. */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

/* rows: row_off [n_entries + 1] into r_word / r_weight, alive [n_entries]; queries likewise by q_off; outputs [n_queries][n_entries] */
void kfdb_ref_query(int n_entries, const int32_t *row_off, const uint8_t *alive, const int32_t *r_word, const double *r_weight, int n_queries,
                    const int32_t *q_off, const int32_t *q_word, const double *q_weight, int32_t *common, double *score)
{
    for (int q = 0; q < n_queries; ++q)
        for (int e = 0; e < n_entries; ++e) {
            const size_t o = (size_t)q * (size_t)n_entries + (size_t)e;
            if (!alive[e]) { common[o] = -1; score[o] = 0.0; continue; }
            int i = q_off[q], j = row_off[e], c = 0;
            const int ie = q_off[q + 1], je = row_off[e + 1];
            double s = 0.0;
            while (i < ie && j < je) {
                if (q_word[i] == r_word[j]) {
                    const double v = q_weight[i], w = r_weight[j];
                    s += fabs(v - w) - fabs(v) - fabs(w);
                    ++c; ++i; ++j;
                } else if (q_word[i] < r_word[j]) ++i;
                else ++j;
            }
            common[o] = c;
            score[o] = -s / 2.0;
        }
}

/* the same terms of one (query, row) pair summed as a pairwise tree (terms 2k and 2k + 1 first, then pairs of those, ...): what a parallel
 * reduction would give.  Used only to show that a fixture tells the two orders apart. */
double kfdb_ref_tree_score(const int32_t *a_word, const double *a_weight, int na, const int32_t *b_word, const double *b_weight, int nb,
                           double *term /* [min(na, nb)] work */)
{
    int i = 0, j = 0, n = 0;
    while (i < na && j < nb) {
        if (a_word[i] == b_word[j]) {
            const double v = a_weight[i], w = b_weight[j];
            term[n++] = fabs(v - w) - fabs(v) - fabs(w);
            ++i; ++j;
        } else if (a_word[i] < b_word[j]) ++i;
        else ++j;
    }
    if (n == 0) return -0.0 / 2.0;
    for (int len = n; len > 1; len = (len + 1) / 2)
        for (int k = 0; k < len / 2 + (len & 1); ++k) term[k] = 2 * k + 1 < len ? term[2 * k] + term[2 * k + 1] : term[2 * k];
    return -term[0] / 2.0;
}
