// ygz/Algorithm/StereoOdometry.h -- ygz::StereoOdometry: frame-to-frame stereo odometry for any number of (current, last) frame pairs in ONE
// device call.  Nothing in the reference, whose tracker is monocular.  It is ORB-SLAM2's TrackWithMotionModel on the last frame's own depths
// (the visual-odometry points of UpdateLastFrame) instead of map points: the last frame's features with a depth are un-projected, searched in
// the current frame with the right-column gate, claimed, checked for orientation, retried at twice the window, and the pose that takes last-camera
// coordinates to current-camera coordinates is optimised over the u, v, uR edges -- all on resident slots, by ygz_hip_stereo_odometry_slots
// (ygz_slam_amd/csrc/svo.hip; the spec is DESIGN.md section 27 and tests/svo_ref.py).  Every pair works in its last camera's frame, so the
// pairs are independent and a whole sequence is one call.
//
// This is odometry: no map is changed, no point is created and no _mappoint is read or written.  StereoTracker (map points, local map) and
// PoseOptimizer stay what they are.
//
// Error conventions of the other surfaces: a failed call logs and returns 0 / false, only a missing device throws.  One thread at a time.
#ifndef YGZ_STEREO_ODOMETRY_H_
#define YGZ_STEREO_ODOMETRY_H_

#include "ygz/Basic.h"

namespace ygz
{

class StereoOdometry
{
public:
    struct Options {
        double _baseline = 0.1;             // metres between the two cameras (what the depths were measured with)
        double _th = 7.0;                   // the window is _th 2^level pixels (ORB-SLAM2's stereo value); doubled for the retry
        int _th_dist = 100;                 // the largest Hamming distance of a match (ORB-SLAM2's TH_HIGH)
        bool _check_orientation = true;     // the rotation histogram
        int _min_matches = 20;              // fewer: one retry with twice the window, then failure
        int _min_tracked = 10;              // fewer inliers: the current frame's pose is left alone
    } _options;

    // what the call answered for one pair
    struct Result {
        int status = 1;                     // 0: tracked (enough matches), 1: too few matches even at twice the window
        int matches = 0, inliers = 0, retried = 0;
        bool pose_written = false;          // status == 0 and inliers >= _min_tracked: current->_TCW was set
        SE3 T_rel;                          // last camera -> current camera, as optimised (the guess when status == 1)
        std::vector<int32_t> match;         // per feature of the last frame: the index of its feature in the current frame, or -1
    };

    StereoOdometry() {}
    explicit StereoOdometry(const Options &options) : _options(options) {}

    // pairs of (current, last).  1. every distinct frame is made resident; 2. its _features (pixel, level -- below 0 counts as 0 --, angle) are
    // described into its slot (ygz_hip_describe_given_angle) and their _depth is set there (ygz_hip_set_keypoint_depths, has_mappoint = depth > 0):
    // whatever keypoints the slot held before are replaced; 3. ONE device call for all pairs, with the guesses (last camera -> current camera;
    // nullptr: the identity for every pair) as entry poses and the motion direction derived from them; 4. for a pair with status 0 and at least
    // _min_tracked inliers, current->_TCW = T_rel * last->_TCW, in pair order (so a chain of pairs in sequence order carries the first frame's
    // pose through); any other pair leaves its current frame alone.  results (may be nullptr) gets one entry per pair.  Returns the number
    // of poses written; 0 with results cleared when the call failed (a null or repeated frame in a pair, a frame with more features than
    // ygz_hip_max_keypoints, guesses of another length, more distinct frames than the runtime has slots, a device error)
    int TrackPairs(const std::vector<std::pair<Frame *, Frame *>> &pairs, const std::vector<SE3> *guesses, std::vector<Result> *results);

    // one pair: TrackPairs of it.  Returns whether current->_TCW was written
    bool Track(Frame *current, Frame *last, const SE3 &guess = SE3(), Result *result = nullptr);
};

}

#endif // YGZ_STEREO_ODOMETRY_H_
