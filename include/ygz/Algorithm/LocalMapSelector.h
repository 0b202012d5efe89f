// ygz/Algorithm/LocalMapSelector.h -- ygz::LocalMapSelector: the local map of any number of frames in ONE device call.  Nothing in the
// reference.  It is ORB-SLAM2's Tracking::UpdateLocalKeyFrames in the form of StereoTracker::LocalKeyFrames (the voters and one covisible
// keyframe of each; no spanning tree, which this data model does not have) and Tracking::UpdateLocalPoints, by ygz_hip_local_map_select
// (ygz_slam_amd/csrc/lms.hip; the spec is DESIGN.md section 34 and tests/lms_ref.c).  It stands between the three calls that give a frame its
// first pose (StereoOdometry, StereoRefTracker, StereoRelocalizer) and StereoLocalMap::TrackLocalMap, which takes the lists it returns: frames
// whose lists are equal get the same list object, so TrackLocalMap sends their point set to the device once.
//
// On every frame it leaves what StereoTracker::LocalKeyFrames leaves when run on the frames one after the other: _ref_keyframe.
// It creates and changes no point and no keyframe.
//
// Error conventions of the other surfaces: a failed call logs and returns 0, only a missing device throws.  One thread at a time.  Every order
// goes by index, list position or id, never by address.
#ifndef YGZ_LOCAL_MAP_SELECTOR_H_
#define YGZ_LOCAL_MAP_SELECTOR_H_

#include "ygz/Basic.h"
#include <memory>

namespace ygz
{

class LocalMapSelector
{
public:
    struct Options {
        int _neighbours = 10;               // the first _neighbours of a voter's _cov_keyframes are looked at (at most 32)
        int _local_keyframes_max = 80;      // the extension stops at this length; the voters alone may exceed it
        int _max_points = 16384;            // points kept per frame; the rest is counted in Result::cut
    } _options;

    // what the call answered for one frame.  The two lists are owned by the selector and stay valid until its next Select
    struct Result {
        const std::vector<Frame *> *keyframes = nullptr;      // StereoTracker::LocalKeyFrames' list; the same object for frames with equal lists
        const std::vector<MapPoint *> *points = nullptr;      // the good map points of those keyframes' features: keyframes in list order,
                                                              // features by index, each point once; shared like `keyframes`
        std::vector<int> prior;                               // per feature of the frame: where its map point stands in `points`, -1 for none
        Frame *ref = nullptr;                                 // the keyframe with the most votes (ties: the smaller _keyframe_id), bad ones included
        int voters = 0;                                       // the keyframes of the list that the frame's points voted for
        int cut = 0;                                          // points beyond _max_points
    };
    struct Stats {
        int frames = 0, keyframes = 0, points = 0, observations = 0;
        int dropped = 0;                    // observations left out: the feature does not point back to the point, is not in its keyframe's
                                            // _features, or its keyframe is already in the point's list
        int lists = 0;                      // distinct keyframe lists among the frames
    };

    LocalMapSelector() {}
    explicit LocalMapSelector(const Options &options) : _options(options) {}

    // 1. The keyframes of the call: every keyframe in the _obs of the frames' good map points (the observing feature's _frame, or
    // Memory::GetKeyFrame of the key, as StereoTracker::LocalKeyFrames finds it) and the first _neighbours entries of those keyframes'
    // _cov_keyframes; indexed in ascending _keyframe_id (equal ids: in the order they were met).  2. The points: the good map points on the
    // frames and on those keyframes' features, each with its observations from _obs and the index of the observing feature in its keyframe;
    // an observation by a keyframe outside (1) is of no consequence and left out; one whose feature does not point back to the point or is
    // not in its keyframe's _features is dropped and counted.  3. ONE device call.  4. Per frame, in frame order: the Result, and
    // _ref_keyframe = ref where there is one.  results (may be nullptr) gets one entry per frame.  Returns the number of frames with a
    // non-empty keyframe list; 0 with results cleared when the call failed (no frame, a null frame, more keyframes, neighbours, frames,
    // observations or features than the call takes, a device error)
    int Select(const std::vector<Frame *> &frames, std::vector<Result> *results);

    const Stats &GetStats() const { return _stats; }

private:
    std::vector<std::unique_ptr<std::vector<Frame *>>> _keyframe_lists;
    std::vector<std::unique_ptr<std::vector<MapPoint *>>> _point_lists;
    Stats _stats;
};

}

#endif // YGZ_LOCAL_MAP_SELECTOR_H_
