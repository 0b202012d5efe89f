// The argument block of k_pose_opt (popt.hip) and its prototype, for the translation units that launch it: popt.hip from host arrays, svo.hip
// from edges a kernel compacted.  The kernel takes only device pointers.
#pragma once
#include "ygz_internal.h"

struct PoptArgs {
    const int32_t *off;                 // [n_frames + 1]; with `end`, [n_frames]: where a frame's edges begin
    const int32_t *end;                 // nullptr: frame f ends at off[f + 1]; else [n_frames], so that the ranges need not touch
    const double *pw, *obs;             // [n][3], [n][3]
    const int32_t *level;
    const uint8_t *kind;
    double *poses;                      // [n_frames][7] in and out
    double *chi2;                       // [n]
    double *cost_initial, *cost_final, *lambda;    // [n_frames][8]
    int32_t *status, *iterations;       // [n_frames][8]
    int32_t *inliers, *rounds_run;      // [n_frames]
    uint8_t *outlier;                   // [n]: the flags of the last classification, read by the passes of the next round
    double K[5];                        // fx fy cx cy bf
    double d2m, d2s, dm, ds;            // chi2_mono, chi2_stereo and their square roots
    double min_rel_decrease;
    int rounds, iters, max_trials, robust_rounds, min_edges, min_inliers;
};

#define PT_DEV_THREADS 256              // one workgroup per frame

__global__ void k_pose_opt(PoptArgs A);
