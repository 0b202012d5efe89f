// ygz/Algorithm/BundleAdjuster.h -- ygz::BundleAdjuster: local and global bundle adjustment for a stereo or RGB-D mapper.  Nothing in the
// reference, whose ba:: functions are monocular, and LoopClosing::GlobalBundleAdjustment has no uR term either: this is ORB-SLAM2's
// Optimizer::LocalBundleAdjustment and GlobalBundleAdjustemnt on this data model -- mono edges (u, v) and stereo edges (u, v, uR) between
// keyframe poses and map points, Huber kernels on chi2, the information scaled by the pyramid level, a robust round, a classification of
// every edge, a second round without kernel and without the outliers -- as one device call (ygz_hip_stereo_ba, ygz_slam_amd/csrc/sba.hip;
// the spec is DESIGN.md section 22 and tests/sba_ref.c).  The third residual, uR - (u - bf / z), is what keeps keyframes and points from
// drifting in scale together; a stereo caller follows LoopClosing::CorrectLoop / FuseLoop with this class's GlobalBundleAdjustment.
//
// Error conventions of the other surfaces: a failed call logs and returns false, only a missing device throws.  One thread at a time.
// Feature, Frame and MapPoint keep their layouts; every order goes by _keyframe_id or index, never by address.
#ifndef YGZ_BUNDLE_ADJUSTER_H_
#define YGZ_BUNDLE_ADJUSTER_H_

#include "ygz/Basic.h"

namespace ygz
{

class BundleAdjuster
{
public:
    struct Options {
        double _baseline = 0.1;         // metres between the two cameras (what u_right was measured with)
        double _chi2_mono = 5.991;      // Huber width and outlier threshold of a mono edge
        double _chi2_stereo = 7.815;    // of a stereo edge
        int _rounds = 2;                // LocalBundleAdjustment: 1 .. 4
        int _robust_rounds = 1;         // the kernel is on in the first _robust_rounds rounds
        int _iterations[4] = { 5, 10, 0, 0 };   // LM iterations of each round, 1 .. 1000
        int _gba_iterations = 10;       // GlobalBundleAdjustment: one robust round of this many
        int _max_trials = 10;
        int _cg_max_iterations = 0;     // 0: min(6 free poses, 1024)
        int _cg_batch = 0;              // 0: 8
        double _cg_tol = 1e-8;
        double _min_rel_decrease = 1e-9;
        bool _erase_outliers = true;    // LocalBundleAdjustment: the outlier edges lose their observation
    } _options;

    // the problem of the last call as handed to ygz_hip_stereo_ba and as it came back; edge e is feature edge_feature[e] of keyframe
    // keyframe_ids[edge_pose[e]] observing point point_ids[edge_point[e]]
    struct Problem {
        vector<unsigned long> keyframe_ids, point_ids;
        vector<double> poses, points, obs;              // [N][7], [L][3], [E][3]
        vector<uint8_t> fixed, kind;                    // [N], [E]
        vector<int32_t> edge_pose, edge_point, level, edge_feature;   // [E]
        double K4[4] = { 0, 0, 0, 0 };
        int points_left_out = 0;                        // points with fewer than two edges
        vector<double> poses_out, points_out, chi2;     // [N][7], [L][3], [E]
        vector<uint8_t> outlier;                        // [E]
    };

    // one round of the last call (YGZ_GBA_* of include/ygz_hip.h in _status)
    struct Round { int _status = 0, _lm_iterations = 0, _n_solves = 0, _cg_iterations = 0, _cg_capped = 0, _inliers = 0; double _cost_initial = 0, _cost_final = 0, _lambda = 0; };
    struct Result { int _rounds_run = 0, _launches = 0; Round _rounds[4]; };     // _launches: kernels the call queued

    BundleAdjuster() {}
    explicit BundleAdjuster(const Options &options) : _options(options) {}

    // the keyframe's stereo columns, copied and kept under its _keyframe_id: StereoMatcher::ComputeStereoMatches' third argument or
    // PoseOptimizer::URightFromDepth.  An observation is a stereo edge when its keyframe has an entry >= 0 at the feature's index, a mono
    // edge otherwise
    void SetURight(const Frame *kf, const std::vector<double> &u_right);
    void ClearURight(const Frame *kf);
    void Clear();

    // LoopClosing::GlobalBundleAdjustment's composition: the keyframes that are not bad, once each, by id, the first fixed; the good map
    // points of their features, each once, with two edges or more among these keyframes; a free keyframe without an edge is refused.  One
    // robust round of _gba_iterations.  _TCW of the free keyframes and _pos_world of the points are rewritten; no observation is erased
    bool GlobalBundleAdjustment(const vector<Frame *> &keyframes);

    // ORB-SLAM2's local BA: free are `keyframe` and its _cov_keyframes that are not bad; the points are the good map points of their features,
    // each once (keyframes by id, features by index); fixed is every other keyframe that is not bad and observes one of them -- if there is
    // none, the free keyframe of smallest id is fixed instead; points with fewer than two edges are left out.  The options' rounds.  On
    // success _TCW of the free keyframes and _pos_world of the points are rewritten and, with _erase_outliers, every outlier edge loses its
    // observation on both sides: the point's _obs entry for that keyframe is erased and Feature::_mappoint set to null; no point is killed,
    // no covisibility recounted.  On an error or a FAILED call: false, and the map is bit-unchanged
    bool LocalBundleAdjustment(Frame *keyframe);

    // the two host halves of the calls above, without a device: the problem of a local (keyframe) or global (keyframes) call into
    // GetProblem(), false when there is nothing to adjust; and the erasure of the gathered problem's edges flagged in outlier [E], which
    // returns the observations erased.  LocalBundleAdjustment is GatherLocal, the device call, the rewrite and EraseOutliers
    bool GatherLocal(Frame *keyframe);
    bool GatherGlobal(const vector<Frame *> &keyframes);
    int EraseOutliers(const std::vector<uint8_t> &outlier);

    const Problem &GetProblem() const { return _problem; }
    const Result &GetResult() const { return _result; }
    int GetOutlierCount() const { return _outlier_count; }

private:
    bool Gather(const vector<Frame *> &free_kfs, bool local, const char *who);
    bool Solve(int rounds, int robust_rounds, const int *iterations, const char *who);

    std::map<unsigned long, std::vector<double>> _u_right;
    Problem _problem;
    Result _result;
    int _outlier_count = 0;
    vector<Frame *> _kfs;               // of the gathered problem: the poses, the points, the edges' features
    vector<MapPoint *> _pts;
    vector<Feature *> _edge_feat;
};

}

#endif // YGZ_BUNDLE_ADJUSTER_H_
