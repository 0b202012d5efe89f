// ygz/Algorithm/LocalMapTracker.h -- ygz::LocalMapTracker: the local map of any number of frames chosen AND tracked with ONE gather of the
// object graph and three device calls.  Nothing in the reference.  It is LocalMapSelector::Select followed by StereoLocalMap::TrackLocalMap
// without the way back through the object graph in between: the map goes to the device once as flat arrays, the attributes of every point
// (Matcher::PointAttributes' normal and dmax) are computed there for the whole map, and a frame's point set is the list of indices the
// selection wrote.  Any number of distinct lists go through one call; the 64 sets of StereoLocalMap do not apply.
//
// It leaves on every frame and every map point what LocalMapSelector::Select and then StereoLocalMap::TrackLocalMap leave.  The host route
// differs in two ways.  A point without a 32-byte descriptor is left out of the set there too (Matcher::PointAttributes refuses it), so the
// two agree; here it is counted in Stats::refused.  A point whose normal or dmax is not finite (it lies on a camera centre) FAILS the whole
// call there (the device refuses a NaN); here it is removed from the lists like any refused point and the call goes on.
// It creates no point and no keyframe.
//
// Error conventions of the other surfaces: a failed call logs and returns 0, only a missing device throws.  One thread at a time.  Every order
// goes by index, list position or id, never by address.
#ifndef YGZ_LOCAL_MAP_TRACKER_H_
#define YGZ_LOCAL_MAP_TRACKER_H_

#include "ygz/Basic.h"
#include "ygz/Algorithm/StereoLocalMap.h"

namespace ygz
{

class LocalMapTracker
{
public:
    struct Options {
        int _neighbours = 10;               // LocalMapSelector's: the first _neighbours of a voter's _cov_keyframes are looked at (at most 32)
        int _local_keyframes_max = 80;      // the extension stops at this length; the voters alone may exceed it
        int _max_points = 16384;            // points kept per frame; the rest is counted in Result::cut
        StereoLocalMap::Options _track;     // StereoLocalMap's
    } _options;

    // StereoLocalMap::Result plus what LocalMapSelector::Result says beside its lists
    struct Result : StereoLocalMap::Result {
        Frame *ref = nullptr;               // the keyframe with the most votes (ties: the smaller _keyframe_id), bad ones included
        int voters = 0;                     // the keyframes of the list that the frame's points voted for
        int cut = 0;                        // points beyond _max_points
        int points = 0;                     // the frame's list after the refused points were removed
    };
    struct Stats {
        int frames = 0, keyframes = 0, points = 0, observations = 0, dropped = 0;      // LocalMapSelector::Stats'
        int centres = 0;                    // distinct observing frames: GetCamCenter() ran once for each
        int attribute_rows = 0;             // observations sent to the attributes call (every usable one, whatever its keyframe)
        int refused = 0;                    // points of the map the attributes refuse: no usable observation, state 2, or no 32-byte descriptor
        int removed = 0;                    // list entries taken out because their point is refused
    };
    // the attributes as they were sent to the tracking call, for the points of the last Track in the order they were met
    struct Sent {
        std::vector<MapPoint *> points;
        std::vector<double> dmax, normal;   // [n], [n][3]
        std::vector<int> state;             // 1: usable
        std::vector<unsigned char> has_desc;
    };

    LocalMapTracker() {}
    explicit LocalMapTracker(const Options &options) : _options(options) {}

    // 1. The gather of LocalMapSelector::Select (its steps 1 and 2), once.  2. The selection, ONE device call.  3. The attributes of every
    // point of the gather, ONE device call: per point ALL usable observations of _obs in key order (feature and its _frame non-null,
    // Matcher::PointAttributes' rule: observers outside the selection's keyframes count, and so do observations whose feature does not point
    // back), the centre from GetCamCenter() once per distinct frame, the level of the observing feature; the descriptor is
    // _distinctive_desc when it holds 32 bytes, else the first usable observation's, copied once per point.  4. A refused point (state != 1 or
    // no descriptor) is removed from the lists on the host, the priors are re-based, the removal is counted.  5. The frames are made
    // resident as StereoLocalMap does, and ONE device call tracks every frame against its list.  6. In frame order, step 4 of
    // StereoLocalMap::TrackLocalMap, and _ref_keyframe = ref where there is one.  results (may be nullptr) gets one entry per frame.
    // Returns the number of frames with status 0 and at least _track._min_tracked inliers; 0 with results cleared when the call failed (no
    // frame, a null or repeated frame, no camera, what LocalMapSelector::Select or StereoLocalMap::TrackLocalMap refuse, a device error)
    int Track(const std::vector<Frame *> &frames, std::vector<Result> *results);

    const Stats &GetStats() const { return _stats; }
    const Sent &GetSent() const { return _sent; }

private:
    Stats _stats;
    Sent _sent;
};

}

#endif // YGZ_LOCAL_MAP_TRACKER_H_
