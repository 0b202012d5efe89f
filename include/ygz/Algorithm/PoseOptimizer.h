// ygz/Algorithm/PoseOptimizer.h -- ygz::PoseOptimizer: the per-frame pose refinement of a stereo or RGB-D tracker.  Nothing in the reference,
// whose ba::OptimizeCurrentPoseOnly is monocular (two residuals on the normalised plane, no robust kernel, no per-level weight): this is
// ORB-SLAM2's Optimizer::PoseOptimization on this data model -- mono edges (u, v) and stereo edges (u, v, uR) against the frame's pose, Huber
// kernels on chi2, the information scaled by the pyramid level, four rounds of ten Levenberg-Marquardt iterations from the entry pose with the
// outliers re-classified in between -- as one device call for any number of frames (ygz_hip_optimize_pose_stereo, ygz_slam_amd/csrc/popt.hip; the
// spec is DESIGN.md section 20 and tests/popt_ref.c).  The third residual, uR - (u - bf / z), is what holds the scale of a stereo tracker.
//
// Error conventions of the other surfaces: a failed call logs and returns 0, only a missing device throws.  One thread at a time.
#ifndef YGZ_POSE_OPTIMIZER_H_
#define YGZ_POSE_OPTIMIZER_H_

#include "ygz/Basic.h"

namespace ygz
{

class PoseOptimizer
{
public:
    struct Options {
        double _baseline = 0.1;         // metres between the two cameras (what u_right was measured with)
        double _chi2_mono = 5.991;      // Huber width and outlier threshold of a mono edge
        double _chi2_stereo = 7.815;    // of a stereo edge
        int _rounds = 4;                // 1 .. 8
        int _iterations = 10;           // LM iterations per round, 1 .. 64
        int _max_trials = 10;           // trials per iteration, 1 .. 64
        int _robust_rounds = 3;         // the kernel is on in the first _robust_rounds rounds
        int _min_edges = 3;
        int _min_inliers = 10;
        double _min_rel_decrease = 0;   // 0: off
    } _options;

    // one round of the last call for a frame (YGZ_POPT_* of include/ygz_hip.h in _status)
    struct Round { int _status; int _lm_iterations; double _cost_initial, _cost_final, _lambda; };

    PoseOptimizer() {}
    explicit PoseOptimizer(const Options &options) : _options(options) {}

    // Every feature of `current` with a good map point (_mappoint set and not _bad) becomes an edge of (_pixel, _level, _mappoint->_pos_world):
    // a stereo edge when u_right is given and its entry for the feature is >= 0 (StereoMatcher::ComputeStereoMatches' third argument, or
    // URightFromDepth), a mono edge otherwise.  On return the frame has what ba::OptimizeCurrentPoseOnly leaves: _TCW, Feature::_bad = outlier
    // for every edge, Feature::_depth of the inliers, _cnt_found of the inliers' map points.  Returns the number of inliers.
    int Optimize(Frame *current, const std::vector<double> *u_right = nullptr);

    // one device call for all frames; u_right has one entry per frame (nullptr: all mono) or is empty
    void OptimizeBatch(const std::vector<Frame *> &frames, const std::vector<const std::vector<double> *> &u_right);

    // uR = u - bf / _depth (bf = the camera's fx times baseline) for the features with _depth > 0, -1 elsewhere: what ORB-SLAM2 does for RGB-D, so
    // that depths from a depth picture give stereo edges too.  Returns the number of entries >= 0.  No device.
    static int URightFromDepth(const Frame *frame, double baseline, std::vector<double> *u_right);

    // of the last call, per frame of the batch: the outlier flag per feature (0 for a feature that was no edge), the rounds that ran, the inliers
    const std::vector<std::vector<uint8_t>> &GetOutliers() const { return _outliers; }
    const std::vector<std::vector<Round>> &GetRounds() const { return _rounds; }
    const std::vector<int> &GetInliers() const { return _inliers; }

private:
    std::vector<std::vector<uint8_t>> _outliers;
    std::vector<std::vector<Round>> _rounds;
    std::vector<int> _inliers;
};

}

#endif // YGZ_POSE_OPTIMIZER_H_
