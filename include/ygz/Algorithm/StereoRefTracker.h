// ygz/Algorithm/StereoRefTracker.h -- ygz::StereoRefTracker: ORB-SLAM2's TrackReferenceKeyFrame for any number of frames in ONE device call.
// Nothing in the reference, whose tracker is monocular.  Every frame is associated with the map points of its reference keyframe by the BoW-guided
// descriptor search (Matcher::SearchByBoW's rules, the claim of Relocalizer, the rotation histogram) and its pose is refined over the u, v, uR
// edges of the associations -- all on resident slots, by ygz_hip_stereo_ref_keyframe_slots (ygz_slam_amd/csrc/srk.hip; the spec is DESIGN.md
// section 29 and tests/srk_ref.py).  It is what a stereo tracker runs on a sequence's first frames, after a relocalisation, without a velocity,
// and when the motion-model search of StereoTracker::TrackWithMotionModel finds too few matches; the associations it leaves are what
// StereoLocalMap::TrackLocalMap takes as the frame's own.
//
// It creates no point and no keyframe; choosing the reference keyframe and the keyframe decisions stay with the caller.
//
// Error conventions of the other surfaces: a failed call logs and returns 0, only a missing device throws.  One thread at a time.
#ifndef YGZ_STEREO_REF_TRACKER_H_
#define YGZ_STEREO_REF_TRACKER_H_

#include "ygz/Basic.h"

namespace ygz
{

class StereoRefTracker
{
public:
    struct Options {
        double _baseline = 0.1;             // metres between the two cameras (what the depths were measured with)
        int _th_low = 50;                   // a match's Hamming distance is below it (ORB-SLAM2's TH_LOW)
        float _knn_ratio = 0.7f;            // best against second best of the same vocabulary node
        int _levelsup = 4;                  // the FeatureVector's node is this many levels above the leaves
        bool _check_orientation = true;     // the rotation histogram removes matches
        int _min_matches = 15;              // fewer associations: the frame is left alone (status 1)
        int _min_inliers = 10;              // fewer inliers after the optimisation: status 2
        int _min_tracked = 10;              // fewer features left with a good observed point: the frame is reported as not tracked
    } _options;

    // what the call answered for one frame
    struct Result {
        int status = 1;                     // 0: optimised, 1: fewer than _min_matches associations, 2: fewer than _min_inliers inliers
        int matches = 0, inliers = 0;       // the associations that went into the optimiser (0 with status 1), its inliers
        int kept = 0;                       // features left with a good map point that a keyframe observes
        bool tracked = false;               // status == 0 and kept >= _min_tracked
    };

    StereoRefTracker() {}
    explicit StereoRefTracker(const Options &options) : _options(options) {}

    // frames[k] is tracked against reference_keyframes[k] from the pose the caller has put into frames[k]->_TCW (ORB-SLAM2: the last frame's);
    // several frames may name one keyframe.  A vocabulary has to be loaded (ORBVocabulary::loadFromBinaryFile / loadFromMemory).
    // 1. A keyframe's set is the good map points of its features by index, each point once; it goes to the device once.  2. Every frame and
    // every keyframe is made resident, its _features (pixel, level -- below 0 counts as 0 --, angle) are described into its slot
    // (ygz_hip_describe_given_angle) and their _depth is set there (ygz_hip_set_keypoint_depths, has_mappoint = depth > 0), as StereoOdometry
    // does: the right columns are u - fx _baseline / _depth.  3. ONE device call.  4. In frame order, what StereoTracker::TrackWithMotionModel's
    // steps 7 to 9 leave: every feature's _mappoint is cleared; with status 1 nothing else happens to the frame; otherwise a matched feature
    // takes its point as _mappoint, _TCW is the optimised pose, a feature whose edge is an outlier gets _bad = true, any other feature with a
    // point _bad = false and its _depth from the new pose (PoseOptimizer::Optimize's effects; the points' _cnt_found is left as it was: found
    // points are counted in TrackLocalMap only), and a _bad feature loses its _mappoint.  results (may be nullptr) gets one entry per frame.
    // Returns the number of tracked frames; 0 with results cleared when the call failed (no frame, lists of another length, a null or
    // repeated frame, a null keyframe, a frame that is its own keyframe, a frame or keyframe with more features than ygz_hip_max_keypoints,
    // more frames than the runtime keeps resident, more keyframes or frames than the call takes, no vocabulary, a device error)
    int TrackReferenceKeyFrame(const std::vector<Frame *> &frames, const std::vector<Frame *> &reference_keyframes, std::vector<Result> *results);
};

}

#endif // YGZ_STEREO_REF_TRACKER_H_
