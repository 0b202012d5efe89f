// The argument block of k_pose_opt (popt.hip), its prototype, and how a launcher fills the block, for the translation units that launch it:
// popt.hip from host arrays, svo.hip, slm.hip and srk.hip from edges a kernel compacted.  The kernel takes only device pointers.
#pragma once
#include "ygz_internal.h"
#include "pose_block.h"

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

// everything of the block that is not a pointer, from checked parameters (ygz_pose_params_ok) and the caller's baseline
inline void ygz_popt_set_params(PoptArgs &G, const double K4[4], double baseline, const ygz_pose_opt_params &q)
{
    for (int k = 0; k < 4; ++k) G.K[k] = K4[k];
    G.K[4] = K4[0] * baseline;
    G.d2m = q.chi2_mono; G.d2s = q.chi2_stereo; G.dm = sqrt(q.chi2_mono); G.ds = sqrt(q.chi2_stereo);
    G.min_rel_decrease = q.min_rel_decrease;
    G.rounds = q.rounds; G.iters = q.iterations; G.max_trials = q.max_trials; G.robust_rounds = q.robust_rounds;
    G.min_edges = q.min_edges; G.min_inliers = q.min_inliers;
}

// the pointers of the block for edges a kernel compacted into the arrays of `b`; frame f's edges begin at off[f] and end at edge_end[f]
inline void ygz_popt_bind(PoptArgs &G, uint8_t *dev, const YgzPoseBlock &b, size_t o_off, size_t o_pose)
{
    G.off = ygz_at<const int32_t>(dev, o_off); G.end = ygz_at<const int32_t>(dev, b.edge_end);
    G.pw = ygz_at<const double>(dev, b.e_pw); G.obs = ygz_at<const double>(dev, b.e_obs);
    G.level = ygz_at<const int32_t>(dev, b.e_level); G.kind = dev + b.e_kind;
    G.poses = ygz_at<double>(dev, o_pose); G.chi2 = ygz_at<double>(dev, b.e_chi2);
    G.cost_initial = ygz_at<double>(dev, b.round_cost_initial); G.cost_final = ygz_at<double>(dev, b.round_cost_final);
    G.lambda = ygz_at<double>(dev, b.round_lambda);
    G.status = ygz_at<int32_t>(dev, b.round_status); G.iterations = ygz_at<int32_t>(dev, b.round_iterations);
    G.inliers = ygz_at<int32_t>(dev, b.inliers); G.rounds_run = ygz_at<int32_t>(dev, b.rounds_run); G.outlier = dev + b.e_outlier;
}
