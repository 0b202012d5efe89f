// ygz/Algorithm/StereoLocalMap.h -- ygz::StereoLocalMap: ORB-SLAM2's TrackLocalMap for any number of frames in ONE device call.  Nothing in the
// reference, whose tracker is monocular.  Every frame is re-associated with the map points of its local keyframes (the LOCAL search with the
// right-column gate, the claim walk with the ratio rule) and its pose is refined over the u, v, uR edges of the associations it came with and
// the new ones -- all on resident slots, by ygz_hip_stereo_local_map_slots (ygz_slam_amd/csrc/slm.hip; the spec is DESIGN.md section 28 and
// tests/slm_ref.py).  It leaves on every frame and every map point what StereoTracker::TrackLocalMap with its PoseOptimizer::Optimize leaves when
// run on the frames one after the other.
//
// It creates no point and no keyframe; keyframe decisions and StereoTracker::LocalKeyFrames stay with the caller.
//
// Error conventions of the other surfaces: a failed call logs and returns 0, only a missing device throws.  One thread at a time.
#ifndef YGZ_STEREO_LOCAL_MAP_H_
#define YGZ_STEREO_LOCAL_MAP_H_

#include "ygz/Basic.h"

namespace ygz
{

class StereoLocalMap
{
public:
    struct Options {
        double _baseline = 0.1;             // metres between the two cameras (what the depths were measured with)
        double _th = 1.0;                   // the window is _th f 2^level pixels, f = _r_near or _r_wide
        double _ratio = 0.8;                // best against second best of the same level
        double _r_near = 2.5;               // the radius factor of a point seen along its normal
        double _r_wide = 4.0;               // of any other point
        double _cos_near = 0.998;           // the viewing cosine above which _r_near applies
        int _th_dist = 100;                 // the largest Hamming distance of a match (ORB-SLAM2's TH_HIGH)
        int _min_edges = 3;                 // fewer associations: the pose is left alone (status 1)
        int _min_tracked = 30;              // fewer inliers: the frame is reported as not tracked
    } _options;

    // what the call answered for one frame
    struct Result {
        int status = 1;                     // 0: optimised, 1: fewer than _min_edges associations
        int new_matches = 0, edges = 0, inliers = 0;
        bool tracked = false;               // status == 0 and inliers >= _min_tracked
    };

    StereoLocalMap() {}
    explicit StereoLocalMap(const Options &options) : _options(options) {}

    // frames[k] is tracked against local_keyframes[k]; frames that are given the same list object share one point set, which goes to the
    // device once.  1. A set is the good map points of its keyframes' features, keyframes in the given order, features by index, each point
    // once, attributes from Matcher::PointAttributes (a refused point is left out).  Unlike StereoTracker::TrackLocalMap the points already on a
    // frame are NOT left out of the set: the call is told about them (prior), skips them for that frame and keeps their features taken.  Every
    // good map point on a frame has to be in that frame's set (it is when the list comes from StereoTracker::LocalKeyFrames), or the call
    // fails.  2. Every frame is made resident, its _features (pixel, level -- below 0 counts as 0 --, angle) are described into its slot
    // (ygz_hip_describe_given_angle) and their _depth is set there (ygz_hip_set_keypoint_depths, has_mappoint = depth > 0), as StereoOdometry
    // does: the right columns are u - fx _baseline / _depth.  3. ONE device call from the frames' _TCW.  4. In frame order, what
    // StereoTracker::TrackLocalMap and PoseOptimizer::Optimize do: _cnt_visible + 1 for every good point on the frame, once; for every other
    // point of the set reason 0: _cnt_visible + 1 and _track_in_view = true, any other reason: false (a point on the frame is not touched); a
    // matched feature takes its point as _mappoint; _TCW is the optimised pose; a feature whose edge is an outlier gets _bad = true, any other
    // feature with a point _bad = false, its _depth from the new pose and its point's _cnt_found + 1.  results (may be nullptr) gets one entry
    // per frame.  Returns the number of frames with status 0 and at least _min_tracked inliers; 0 with results cleared when the call failed (no
    // frame, lists of another length, a null or repeated frame, a frame with more features than ygz_hip_max_keypoints, more frames than the
    // runtime keeps resident, a point on a frame that its set does not hold, more sets, frames or pairs than the call takes, a device error)
    int TrackLocalMap(const std::vector<Frame *> &frames, const std::vector<const std::vector<Frame *> *> &local_keyframes,
                      std::vector<Result> *results);
};

}

#endif // YGZ_STEREO_LOCAL_MAP_H_
