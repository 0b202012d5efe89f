// The argument block of the three P3P RANSAC kernels (pnp.hip) and their prototypes, for the translation units that launch them: pnp.hip from
// host arrays, srl.hip from associations a kernel compacted.  The kernels take only device pointers.  They live in a named namespace, so that
// their symbols read ...k_pnp_solveE... in every translation unit.
#pragma once
#include "ygz_internal.h"

#define PNP_SOLVE_LANES 64                 // k_pnp_solve
#define PNP_SCORE_LANES 256                // k_pnp_score: hypotheses per block = points per LDS tile
#define PNP_SEL_THREADS 256                // k_pnp_select

namespace ygz_pnp {

struct PnpIn {
    double K4[4];
    double chi2;
    int32_t n_problems, max_iter, min_inliers, pad;
};

struct PnpDev {
    const PnpIn *in;
    const int32_t *off;               // [P + 1]; with `end`, [P]: where a problem's points begin
    const double *pw, *px;            // [N][3], [N][2]
    const int32_t *sets;              // [P][max_iter][3]
    // the block that is copied back
    ygz_pnp_result *res;              // [P]
    uint8_t *mask;                    // [N]
    int32_t *nsol;                    // [P][max_iter]
    int32_t *counts;                  // [P][max_iter][4]
    double *sol;                      // [P][max_iter][4][12]
    const int32_t *end;               // nullptr: problem p ends at off[p + 1]; else [P], a device row, so that the ranges need not touch
    const int32_t *skip;              // nullptr: none; else [P], non-zero: the problem gets no hypothesis (its sample sets are not read)
};

// grid (samples / 64, problems); grid (4 * max_iter / 256, problems); grid (problems)
__global__ void k_pnp_solve(PnpDev D);
__global__ void k_pnp_score(PnpDev D);
__global__ void k_pnp_select(PnpDev D);

}  // namespace ygz_pnp
