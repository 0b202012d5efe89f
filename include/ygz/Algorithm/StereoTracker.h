// ygz/Algorithm/StereoTracker.h -- ygz::StereoTracker: the data association of a stereo or RGB-D tracker.  Nothing in the reference, whose
// tracker is monocular and semi-direct (LK, sparse alignment, FindDirectProjection): it never reads a right column and its descriptor-free
// association cannot keep a near point out of a far keypoint at the same pixel.  These are ORB-SLAM2's two tracking searches on this data
// model, both on one device primitive with the right-column gate (ygz_hip_stereo_track_search, ygz_slam_amd/csrc/strack.hip; the spec is
// DESIGN.md section 26 and tests/strack_ref.c):
//   TrackWithMotionModel  Tracking::TrackWithMotionModel: the pose predicted from the velocity, ORBmatcher::SearchByProjection(CurrentFrame,
//                         LastFrame, th, bMono) with the retry at twice the window, PoseOptimizer, the outliers dropped;
//   LocalKeyFrames        Tracking::UpdateLocalKeyFrames WITHOUT the spanning tree: this data model has no parent and no children of a
//                         keyframe, so only the voters and one covisible neighbour of each enter;
//   TrackLocalMap         Tracking::SearchLocalPoints + TrackLocalMap: the visible / found counters that StereoMapper::MapPointCulling
//                         reads, ORBmatcher::SearchByProjection(F, vpMapPoints, th), PoseOptimizer.
// After it a caller can run rectify -> stereo match -> track -> pose optimise -> keyframe -> create / fuse / BA / cull.  Not here:
// UpdateLastFrame's temporary points, NeedNewKeyFrame, TrackReferenceKeyFrame (StereoRefTracker, ygz/Algorithm/StereoRefTracker.h, serves).
//
// Error conventions of the other surfaces: a failed call logs and returns 0, only a missing device throws.  One thread at a time.  Feature,
// Frame and MapPoint keep their layouts; every order goes by index, list position or id, never by address.
#ifndef YGZ_STEREO_TRACKER_H_
#define YGZ_STEREO_TRACKER_H_

#include "ygz/Basic.h"

namespace ygz
{

class PoseOptimizer;

class StereoTracker
{
public:
    struct Options {
        double _baseline = 0.1;             // metres between the two cameras (what the right columns were measured with)
        double _th_motion = 7.0;            // TrackWithMotionModel: the window is _th_motion 2^level pixels (ORB-SLAM2's stereo value; a mono caller sets 15)
        double _th_local = 1.0;             // TrackLocalMap: the window is _th_local f 2^level pixels, f = 2.5 or 4 (RGB-D: 3)
        int _th_dist = 100;                 // the largest Hamming distance of a match (ORB-SLAM2's TH_HIGH)
        double _ratio = 0.8;                // TrackLocalMap: best against second best of the same level
        bool _check_orientation = true;     // TrackWithMotionModel: the rotation histogram
        int _min_matches_motion = 20;       // fewer: one retry with twice the window
        int _local_keyframes_max = 80;
        int _neighbours = 10;               // LocalKeyFrames: the first _neighbours of a voter's _cov_keyframes are looked at
    } _options;

    // what one device call saw and answered: the points of its set in set order, their attributes as uploaded (level and angle: FRAME; dmax
    // and normal: LOCAL), the current frame's kp_taken, and per point the outputs of ygz_hip_stereo_track_search
    struct Search {
        std::vector<MapPoint *> points;
        std::vector<double> pw, dmax, normal, angle, proj;
        std::vector<uint8_t> desc, taken;
        std::vector<int32_t> level, match, dist, reason, outcome, n_cand, n_gated;
        int32_t counts[4] = { 0, 0, 0, 0 };         // matches, searched, overflowed, removed by orientation
        double T[7] = { 0, 0, 0, 1, 0, 0, 0 };      // current's pose as searched
        double th = 0;
        int direction = 0;
    };
    struct Stats {
        int direction = 0, retried = 0;                                             // of the last TrackWithMotionModel
        int motion_points = 0, motion_matches = 0, motion_inliers = 0, motion_kept = 0;
        int local_keyframes = 0, local_on_frame = 0, local_points = 0, local_cut = 0, local_searched = 0, local_matches = 0, local_inliers = 0,
            local_kept = 0;
    };

    StereoTracker() {}
    explicit StereoTracker(const Options &options) : _options(options) {}

    // the frame's right columns, copied and kept under its _id (tracked frames are not keyframes): a feature is a stereo keypoint when its
    // frame has an entry >= 0 at the feature's index, a mono keypoint otherwise
    void SetURight(const Frame *frame, const std::vector<double> &u_right);
    void ClearURight(const Frame *frame);
    void Clear();

    // 1. current->_TCW = velocity last->_TCW; 2. every _mappoint of current is cleared; 3. the point set: last's features with a good map point
    // and _bad == false, in feature order, attributes of Matcher::PointAttributes (a refused point is skipped), pt_level the feature's _level
    // (below 0 counts as 0), pt_angle its _angle; 4. the direction from t_lc = R_l (-R_c^T t_c) + t_l: +1 when t_lc.z > _baseline, -1 when
    // -t_lc.z > _baseline, 0 otherwise and for a current frame without any right column; 5. one device call with th = _th_motion; 6. fewer
    // than _min_matches_motion matches: one more call with 2 _th_motion; still fewer: returns 0, the pose stays the prediction and current has
    // no map points; 7. the matched features get _mappoint; 8. opt.Optimize(current, current's columns) with the matched points' _cnt_found
    // saved and restored (found points are counted in TrackLocalMap only); 9. a feature the optimiser marked _bad loses its _mappoint.
    // Returns the number of features left with a good map point that has an observation (the caller compares it with 10)
    int TrackWithMotionModel(Frame *current, Frame *last, const SE3 &velocity, PoseOptimizer &opt);

    // Host code.  Every keyframe in the _obs of current's good map points gets a vote; the voters that are not bad enter in _keyframe_id
    // order; then, for each of those in order, the first of its first _neighbours _cov_keyframes that is not bad and not in the list enters,
    // until _local_keyframes_max.  current->_ref_keyframe = the voter with the most votes (ties: the smaller id).  ORB-SLAM2 also adds a
    // voter's children and parent in the spanning tree: this data model has none.  Returns the length of *out
    int LocalKeyFrames(Frame *current, std::vector<Frame *> *out);

    // 1. every good map point already on current: _cnt_visible + 1; 2. the point set: the good map points of the local keyframes' features,
    // keyframes in the given order, features by index, each once, those already on current left out (above YGZ_STRACK_MAX_PAIRS the list is
    // cut and the cut counted); 3. attributes of Matcher::PointAttributes; 4. one LOCAL problem of current's keypoints, those with a good map
    // point taken; 5. ONE device call with th = _th_local; 6. reason 0: _cnt_visible + 1 and _track_in_view = true, any other reason:
    // _track_in_view = false; 7. a match sets the feature's _mappoint; 8. opt.Optimize, which raises _cnt_found of the inliers; 9. returns the
    // number of features with a good, observed map point and _bad == false (the caller compares it with 30).  _last_seen is not written: the
    // mapper keeps keyframe ids there
    int TrackLocalMap(Frame *current, const std::vector<Frame *> &local_keyframes, PoseOptimizer &opt);

    const Search &GetSearch(int which) const { return _search[which ? 1 : 0]; }      // 0: the last motion call (the retry when there was one), 1: local
    const Stats &GetStats() const { return _stats; }

private:
    const std::vector<double> *Columns(const Frame *frame) const;
    bool Run(Frame *current, Search &s, int mode, const char *what);

    std::map<unsigned long, std::vector<double>> _u_right;
    Search _search[2];
    Stats _stats;
};

}

#endif // YGZ_STEREO_TRACKER_H_
