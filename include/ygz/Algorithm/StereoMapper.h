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
//   SearchInNeighbors     LocalMapping::SearchInNeighbors: the keyframe's points are fused into its neighbours and their neighbours and the
//                         neighbours' points into the keyframe (ORBmatcher::Fuse with th = 3 in both directions: the projection has to lie
//                         within chi2 of the keypoint, the right column included on a stereo keypoint; ygz_hip_local_fuse_search, ONE call
//                         per direction), so that one landmark is one MapPoint again;
//   MapPointCulling       LocalMapping::MapPointCulling: the recently created points that never earn observations are set bad (host code).
// Their spec is DESIGN.md section 25 and tests/lfuse_ref.c.  The mapper's loop is create, fuse, local BA, cull keyframes.
//
// Error conventions of the other surfaces: a failed call logs and returns 0 and the map is left unchanged, only a missing device throws.  One
// thread at a time.  A feature whose map point is bad counts as free: when it receives a new point it is first erased from the bad point's
// _obs, so no observation names a feature that points elsewhere.  Feature, Frame and MapPoint keep their layouts; every order goes by _keyframe_id or index, never by address.
#ifndef YGZ_STEREO_MAPPER_H_
#define YGZ_STEREO_MAPPER_H_

#include "ygz/Basic.h"

namespace ygz
{

class Matcher;

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
        int _neighbours = 10;               // CreateNewMapPoints, SearchInNeighbors: the first _neighbours of _cov_keyframes that are not bad
        int _second_neighbours = 5;         // SearchInNeighbors: the first of each neighbour's own _cov_keyframes
        double _fuse_th = 3.0;              // SearchInNeighbors: the search window is _fuse_th 2^level pixels
        double _fuse_chi2_mono = 5.99;      // the gate of a mono and of a stereo keypoint, scaled by 4^level: ORB-SLAM2's constants in Fuse
        double _fuse_chi2_stereo = 7.8;
        int _cull_min_obs = 3;              // MapPointCulling: ORB-SLAM2's stereo value; a mono caller sets 2
        float _cull_found_ratio = 0.25f;
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

    // ---- local-map fusion
    enum FusionKind { FUSE_ADDED = 0, FUSE_REPLACED_INTO_POINT = 1, FUSE_REPLACED_INTO_FEATURE = 2, FUSE_CONFLICT = 3 };
    // one action of the walk: the hit (target keyframe id, point id as searched, feature index) and the point that survives
    struct Fusion { int kind; unsigned long target; unsigned long point; int feature; unsigned long survivor; };
    struct FuseStats {
        int targets = 0, targets_dropped = 0;           // targets beyond YGZ_LFUSE_MAX_PROBLEMS (64) are dropped
        int forward_points = 0, forward_hits = 0, reverse_points = 0, reverse_cut = 0, reverse_hits = 0;
        int added = 0, replaced = 0, conflicts = 0, descriptors = 0;
    };
    // what one of the two device calls saw and answered: the points of its set (in set order), their attributes as uploaded, per problem the
    // pt_skip flags and the matches (feature index or -1), both [problems][points]
    struct Search {
        std::vector<MapPoint *> points;
        std::vector<double> pw, dmax, normal;
        std::vector<uint8_t> desc, skip;
        std::vector<int32_t> match;
    };

    // 1. targets, ORB-SLAM2's interleaved walk: the first _neighbours entries of kf->_cov_keyframes that are not bad, in order; each becomes a
    //    target unless it already is one, and directly after it the first _second_neighbours entries of ITS _cov_keyframes that are not bad, not
    //    kf and not already a target.  Targets beyond 64 are dropped and counted.
    // 2. forward: ONE point set, kf's good map points by feature index, each once, with Matcher::PointAttributes (a point it refuses is
    //    skipped); one problem per target (_TCW; _pixel, _level -- below 0 counts as 0 --, _desc; kp_ur from SetURight's table or -1; pt_skip
    //    where the point's _obs already holds the target's keyframe id); ONE device call for all targets.
    // 3. the walk: targets in order, then points by index; each hit (target k, point i, feature f) is re-checked against the map as it is NOW.
    //    P = the survivor of point i (replacements made earlier in this walk are followed).  P bad or already observed by k: a conflict,
    //    nothing changes.  q = f->_mappoint: q null or bad -> P->_obs[k id] = f, f->_mappoint = P (a bad q first loses f from its _obs);
    //    q = P -> nothing; otherwise with nObs counting a stereo side 2 and a mono side 1 (ORB-SLAM2's Observations()): nObs(q) > nObs(P) ->
    //    LoopClosing::ReplaceMapPoint(P, q), else (a tie included) ReplaceMapPoint(q, P).
    //    (The one difference from ORB-SLAM2, which fuses target by target: there target k is searched on the map that target k-1 already
    //    changed; here all targets are searched on the map as it stood, and the walk re-checks every hit.)
    // 4. reverse: the good map points of the targets' features, targets in order, features by index, each once, on the map after step 3 (more
    //    than YGZ_LFUSE_MAX_PAIRS: the first that many, the cut is counted); one problem, kf; ONE device call; the same walk.
    // 5. matcher.ComputeDistinctiveDescriptors once over kf's good points.  Covisibility is NOT recounted: GetTouched() has, by id, the
    //    keyframes in which some feature's _mappoint changed or that gained an observation, and the caller runs
    //    LoopClosing::UpdateCovisibility(touched, keyframes).
    // Returns the number of fusions: observations added plus replacements.  A failed device call logs and returns 0; the map is unchanged when
    // it is the forward call (parameters and capacities are refused there), and keeps step 3's fusions when the device fails in the reverse call.
    int SearchInNeighbors(Frame *kf, Matcher &matcher);
    const std::vector<Fusion> &GetFusions() const { return _fusions; }          // every action of the last call, in order
    const std::vector<Frame *> &GetTouched() const { return _touched; }
    const std::vector<Frame *> &GetTargets() const { return _targets; }
    const FuseStats &GetStats() const { return _fuse_stats; }
    const Search &GetSearch(int reverse) const { return _search[reverse ? 1 : 0]; }

    // Pure host code.  CreateKeyframePoints and CreateNewMapPoints append what they create to a list of recent points.  With c =
    // kf->_keyframe_id the list is walked in order; per point p: p bad -> dropped from the list; _cnt_visible > 0 && GetFoundRatio() <
    // _cull_found_ratio -> set bad and dropped; c >= _first_seen + 2 && nObs(p) <= _cull_min_obs -> set bad and dropped; c >= _first_seen + 3
    // -> dropped (it survived).  Setting bad is ORB-SLAM2's SetBadFlag: every _obs feature gets _mappoint = nullptr, _obs is cleared, _bad =
    // true.  Returns the number of points set bad
    int MapPointCulling(Frame *kf);
    const std::vector<MapPoint *> &GetRecent() const { return _recent; }
    void ClearRecent() { _recent.clear(); }

private:
    double URight(const Frame *kf, size_t index) const;

    std::map<unsigned long, std::vector<double>> _u_right;
    std::vector<int32_t> _codes, _methods, _pair_neighbour;
    std::vector<std::pair<int, int>> _pairs;
    std::vector<Frame *> _neighbours;
    std::vector<MapPoint *> _created;

    int Observations(const MapPoint *mp) const;          // a stereo side counts 2, a mono side 1
    int Walk(const std::vector<Frame *> &targets, const Search &s, std::set<Frame *> &touched);
    std::vector<MapPoint *> _recent;
    std::vector<Fusion> _fusions;
    std::vector<Frame *> _touched, _targets;
    FuseStats _fuse_stats;
    Search _search[2];
};

}

#endif // YGZ_STEREO_MAPPER_H_
