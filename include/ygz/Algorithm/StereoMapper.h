// ygz/Algorithm/StereoMapper.h -- ygz::StereoMapper: map-point creation for a stereo or RGB-D mapper.  Nothing in the reference, whose
// LocalMapping::CreateNewMapPoints (src/Module/LocalMapping.cpp:375-495) is monocular: it needs ray parallax between two keyframes, re-aligns
// pixels photometrically and never reads a right column.  These are ORB-SLAM2's two creation paths on this data model:
//   CreateKeyframePoints  Tracking::StereoInitialization / CreateNewKeyFrame: the keyframe's own features with a depth, nearest first, the close
//                         ones and at least _min_close of them un-projected into the world (ygz_hip_stereo_keyframe_points);
//   CreateNewMapPoints    LocalMapping::CreateNewMapPoints with stereo: the matches with the best covisible keyframes, each triangulated or
//                         un-projected from the better of its two stereo measurements, then tested for positive depth, reprojection with the
//                         uR term and scale consistency (ygz_hip_stereo_create_map_points, ONE call for all neighbours).
// The spec is DESIGN.md section 24 and tests/smap_ref.c.  Neither call recounts covisibility or recomputes distinctive descriptors:
// ygz_hip_covisibility and ygz_hip_distinctive_descriptors exist and the caller composes them.
//
// Error conventions of the other surfaces: a failed call logs and returns 0 and the map is left unchanged, only a missing device throws.  One
// thread at a time.  A feature whose map point is bad counts as free: when it receives a new point it is first erased from the bad point's
// _obs, so no observation names a feature that points elsewhere.  Feature, Frame and MapPoint keep their layouts; every order goes by _keyframe_id or index, never by address.
#ifndef YGZ_STEREO_MAPPER_H_
#define YGZ_STEREO_MAPPER_H_

#include "ygz/Basic.h"

namespace ygz
{

class StereoMapper
{
public:
    struct Options {
        double _baseline = 0.1;             // metres between the two cameras (what u_right and the depths were measured with)
        double _chi2_mono = 5.991;          // reprojection thresholds of a mono and of a stereo side, scaled by 4^level
        double _chi2_stereo = 7.8;          // ORB-SLAM2's value in this function
        double _cos_parallax_max = 0.9998;  // two mono sides are triangulated below it only
        double _th_depth = 3.5;             // metres: a keyframe's feature up to it is close
        int _min_close = 100;               // at least this many of the nearest features are walked
        int _neighbours = 10;               // CreateNewMapPoints: the first _neighbours of _cov_keyframes that are not bad
    } _options;

    StereoMapper() {}
    explicit StereoMapper(const Options &options) : _options(options) {}

    // the keyframe's stereo columns, copied and kept under its _keyframe_id (BundleAdjuster's convention): a feature is a stereo side when its
    // keyframe has an entry >= 0 at the feature's index, a mono side otherwise.  The depth of a stereo side is Feature::_depth as it stands: it
    // must be the depth that entry was measured with (what StereoMatcher::ComputeStereoMatches leaves in both).  CreateNewMapPoints writes the
    // _depth of MONO sides; a caller that later supplies a u_right entry for such a feature sets its _depth with it
    void SetURight(const Frame *kf, const std::vector<double> &u_right);
    void ClearURight(const Frame *kf);
    void Clear();

    // One device call over kf->_features (_pixel, _depth, has a good map point).  Every selected feature, in feature order, gets a new map point:
    // _first_seen = _last_seen = kf's keyframe id, _obs[that id] = the feature, _cnt_visible = _cnt_found = 1, _pos_world, _bad = false, and the
    // feature points at it.  Returns the number created
    int CreateKeyframePoints(Frame *kf);

    // The first _neighbours of kf->_cov_keyframes that are not bad; one closer than _baseline between the camera centres is skipped (ORB-SLAM2's
    // stereo rule).  Per neighbour E12 as the reference forms it and Matcher::SearchForTriangulation, unchanged; pairs of which a feature has a
    // good map point are dropped; one device call for all neighbours; then, in neighbour order and pair order, a code-0 pair becomes a map point
    // unless one of its two features received a point earlier in this walk.  (The one difference from ORB-SLAM2, which matches neighbour by
    // neighbour: there, a feature that got a point from an earlier neighbour is not offered to a later neighbour's matcher; here it is matched
    // again and the walk refuses the second point.)  A new map point
    // gets _first_seen = _last_seen = kf's keyframe id, both _obs entries, _cnt_visible = _cnt_found = 2, _pos_world; both features point at it
    // with _bad = false, and Feature::_depth of a MONO side is set to the point's z in that camera.  Returns the number created
    int CreateNewMapPoints(Frame *kf);

    // the last call: per pair of the device call its code and method (include/ygz_hip.h), the neighbour it belongs to (index into GetNeighbours())
    // and its two feature indices; the neighbours that were matched; the map points made, in creation order
    const std::vector<int32_t> &GetCodes() const { return _codes; }
    const std::vector<int32_t> &GetMethods() const { return _methods; }
    const std::vector<Frame *> &GetNeighbours() const { return _neighbours; }
    const std::vector<MapPoint *> &GetCreated() const { return _created; }
    const std::vector<int32_t> &GetPairNeighbour() const { return _pair_neighbour; }
    const std::vector<std::pair<int, int>> &GetPairs() const { return _pairs; }

private:
    double URight(const Frame *kf, size_t index) const;

    std::map<unsigned long, std::vector<double>> _u_right;
    std::vector<int32_t> _codes, _methods, _pair_neighbour;
    std::vector<std::pair<int, int>> _pairs;
    std::vector<Frame *> _neighbours;
    std::vector<MapPoint *> _created;
};

}

#endif // YGZ_STEREO_MAPPER_H_
