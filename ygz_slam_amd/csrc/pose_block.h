// The host plumbing the entry points that launch k_pose_opt share: the range check of ygz_pose_opt_params, the finiteness check of an input
// array, the place of the pose-result and edge arrays in a packed block, and the list of a call's distinct slots.  Plain C++ without a HIP
// header, so a host program can include it (tests/cpp/pose_block_host.cpp).
#pragma once
#include <math.h>
#include <string.h>
#include <vector>
#include "../../include/ygz_hip.h"
#include "ygz_blob.h"

inline bool ygz_all_finite(const double *v, size_t n)
{
    for (size_t i = 0; i < n; ++i) if (!isfinite(v[i])) return false;
    return true;
}

// what every launcher of k_pose_opt asks of the parameters; the baseline is the caller's to judge
inline bool ygz_pose_params_ok(const ygz_pose_opt_params &p)
{
    if (!isfinite(p.chi2_mono) || !isfinite(p.chi2_stereo) || !isfinite(p.min_rel_decrease)) return false;
    return p.chi2_mono > 0.0 && p.chi2_stereo > 0.0 && p.rounds >= 1 && p.rounds <= YGZ_POPT_MAX_ROUNDS && p.iterations >= 1 &&
           p.iterations <= YGZ_POPT_MAX_STEPS && p.max_trials >= 1 && p.max_trials <= YGZ_POPT_MAX_STEPS;
}

// the offsets of k_pose_opt's seven result arrays for F frames, and of the eight edge arrays of F frames of `cells` entries each
struct YgzPoseBlock {
    size_t inliers, rounds_run, round_status, round_iterations, round_cost_initial, round_cost_final, round_lambda;
    size_t edge_of, e_pw, e_obs, e_level, e_kind, e_outlier, e_chi2, edge_end;
    void add_results(YgzBlobLayout &B, size_t F)
    {
        const size_t R8 = F * YGZ_POPT_MAX_ROUNDS;
        inliers = B.add_n<int32_t>(F); rounds_run = B.add_n<int32_t>(F); round_status = B.add_n<int32_t>(R8);
        round_iterations = B.add_n<int32_t>(R8);
        round_cost_initial = B.add_n<double>(R8); round_cost_final = B.add_n<double>(R8); round_lambda = B.add_n<double>(R8);
    }
    void add_edges(YgzBlobLayout &B, size_t F, size_t cells)
    {
        const size_t N = F * cells;
        edge_of = B.add_n<int32_t>(N);
        e_pw = B.add_n<double>(N * 3); e_obs = B.add_n<double>(N * 3); e_level = B.add_n<int32_t>(N); e_kind = B.add_n<uint8_t>(N);
        e_outlier = B.add_n<uint8_t>(N); e_chi2 = B.add_n<double>(N); edge_end = B.add_n<int32_t>(F);
    }
    // the results from the host copy `up` of the block to the caller's arrays, each of which may be absent
    void copy_results(const uint8_t *up, size_t F, int32_t *inliers_, int32_t *rounds_run_, int32_t *round_status_, int32_t *round_iterations_,
                      double *round_cost_initial_, double *round_cost_final_, double *round_lambda_) const
    {
        const size_t R8 = F * YGZ_POPT_MAX_ROUNDS;
        if (inliers_) memcpy(inliers_, up + inliers, F * 4);
        if (rounds_run_) memcpy(rounds_run_, up + rounds_run, F * 4);
        if (round_status_) memcpy(round_status_, up + round_status, R8 * 4);
        if (round_iterations_) memcpy(round_iterations_, up + round_iterations, R8 * 4);
        if (round_cost_initial_) memcpy(round_cost_initial_, up + round_cost_initial, R8 * 8);
        if (round_cost_final_) memcpy(round_cost_final_, up + round_cost_final, R8 * 8);
        if (round_lambda_) memcpy(round_lambda_, up + round_lambda, R8 * 8);
    }
};

// the place of slot s in the list of a call's distinct slots, appended on first sight; `where` has an entry of -1 for every slot of the context
inline int32_t ygz_distinct_slot(std::vector<int32_t> &slots, std::vector<int32_t> &where, int32_t s)
{
    if (where[(size_t)s] < 0) { where[(size_t)s] = (int32_t)slots.size(); slots.push_back(s); }
    return where[(size_t)s];
}
