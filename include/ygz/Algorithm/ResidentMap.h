// ygz/Algorithm/ResidentMap.h -- ygz::ResidentMap: the map of LocalMapTracker with a home in device memory, and the local map of any number
// of frames chosen AND tracked on it in ONE device call.  Nothing in the reference.  LocalMapTracker sends the map
// three times per call; a tracker works on one frame at a time and the map changes at keyframe rate, so here it goes up when it changes
// (Upload, or Update after a bundle adjustment or a culling) and Track sends only the frames' point entries and poses.
//
// When the two routes agree.  LocalMapTracker::Track gathers its universe from the frames: the keyframes that observe a point on a frame,
// and the first _neighbours entries of their _cov_keyframes.  ResidentMap::Track leaves on every frame and every map point what
// LocalMapTracker::Track leaves, bit for bit, when the resident universe CONTAINS that one: the frames' observers and their first _neighbours
// covisible keyframes.  Selection reads nothing else (votes go to observers, the extension looks at the voters' covisible rows, the point set
// is what the listed keyframes carry), so a superset changes no outcome.  A feature whose point the map does not hold is sent as "no point"
// and counted in Stats::unknown; LocalMapTracker would have gathered that point.
//
// What makes the resident map stale.  Anything Upload read and Update does not push: a new keyframe, a new or erased observation, a changed
// _cov_keyframes list, a new map point, a changed feature level -- these need a new Upload.  A moved point or keyframe, a new descriptor and
// a changed _bad flag are pushed by Update.  Track reads the map as the device holds it and never looks at the keyframes again.
//
// Error conventions of the other surfaces: a failed call logs and returns 0 (false), only a missing device throws.  One thread at a time.
// Every order goes by index, list position or id, never by address.
#ifndef YGZ_RESIDENT_MAP_H_
#define YGZ_RESIDENT_MAP_H_

#include "ygz/Basic.h"
#include "ygz/Algorithm/LocalMapTracker.h"

namespace ygz
{

class ResidentMap
{
public:
    typedef LocalMapTracker::Options Options;       // _neighbours, _local_keyframes_max, _max_points, _track
    typedef LocalMapTracker::Result Result;
    Options _options;

    struct Stats {
        int keyframes = 0, points = 0, observations = 0, dropped = 0;      // of the last Upload: LocalMapSelector::Stats'
        int centres = 0, attribute_rows = 0;                                // of the last Upload: LocalMapTracker::Stats'
        int refused = 0;                    // points the resident attributes refuse, as of the last Upload
        int uploads = 0, updates = 0;       // accepted ones
        int skipped = 0;                    // objects the last Update was given that the map does not hold
        int frames = 0;                     // of the last Track
        int unknown = 0;                    // features of the last Track's frames whose point the map does not hold
        int removed = 0;                    // list entries of the last Track taken out because their point is refused
    };

    ResidentMap();
    explicit ResidentMap(const Options &options);
    ~ResidentMap();
    ResidentMap(const ResidentMap &) = delete;
    ResidentMap &operator=(const ResidentMap &) = delete;

    // Makes the map of these keyframes resident, by LocalMapTracker's rules: the keyframes ordered by _keyframe_id (null and repeated entries
    // skipped), their first _neighbours _cov_keyframes inside the list, the points on their features in the order they are met, the
    // observations that mirror the keyframes' features for the selection, every usable observation in key order with one centre per distinct
    // frame for the attributes, the descriptor by LocalMapTracker's rule.  Keeps the point and keyframe tables.  false: nothing usable, or the
    // device refused; the map that was resident before stays.
    bool Upload(const std::vector<Frame *> &keyframes);

    // Pushes the positions, descriptors and bad flags of these points and the bad flags and camera centres of these keyframes; the device
    // recomputes every attribute.  An object the map does not hold is counted in Stats::skipped and skipped.  Returns the number of objects
    // pushed; 0 also when the call failed or nothing was resident.
    int Update(const std::vector<MapPoint *> &points, const std::vector<Frame *> &keyframes);

    // LocalMapTracker::Track on the resident map with ONE device call: the frames are made resident, their features' points are looked up
    // (-1 for a point the map does not hold), and the answer is applied as LocalMapTracker::Track's step 6 applies it: _cnt_visible,
    // _cnt_found and _track_in_view, the new _mappoints, _TCW, the optimiser's verdicts and _ref_keyframe.  Returns the number of frames
    // with status 0 and at least _track._min_tracked inliers; 0 with results cleared when the call failed (no frame, a null or repeated
    // frame, no camera, no resident map, a frame with more features than the context has cells, a device error).
    int Track(const std::vector<Frame *> &frames, std::vector<Result> *results);

    bool Resident() const;
    const Stats &GetStats() const { return _stats; }

private:
    struct Impl;
    Impl *_impl;
    Stats _stats;
};

}

#endif // YGZ_RESIDENT_MAP_H_
