// What the class surfaces under host/ share (surface_share.cpp).  Private to libygz_host.so like fdp_memo.h: gathers of
// Frame / Feature / MapPoint fields into the flat arrays the C ABI takes, the loading of feature lists into resident slots, and the per-feature
// effect of a pose optimisation.  Host code only; the slot loader alone reaches the Runtime, and only after its input has been checked.
#ifndef YGZ_HOST_SURFACE_SHARE_H_
#define YGZ_HOST_SURFACE_SHARE_H_
#include "ygz/Basic.h"
namespace ygz {
namespace hip {
inline bool good(const MapPoint *mp) { return mp && !mp->_bad; }

// a frame's feature list as ygz_hip_describe_given_angle and ygz_hip_set_keypoint_depths take it: _pixel, _level (below 0 counts as 0), _angle as
// float, _depth, and has = _depth > 0.  Every feature is non-null
struct FeatureArrays {
    std::vector<double> px, depth;
    std::vector<int32_t> level;
    std::vector<float> angle;
    std::vector<uint8_t> has;
    explicit FeatureArrays(const Frame *f);
};

// what would refuse a list of frames: a null frame, a null feature, more features than `cells`.  Logs under `who`; nothing is touched
bool loadable(const char *who, const std::vector<Frame *> &frames, size_t cells);
// the frames into resident slots, in the given order (slots are assigned least recently used), each with its feature list and depths; slot gets
// one entry per frame.  loadable() is asked before the first device call.  false: logged under `who`, the caller returns its failure value
bool load_slots(const char *who, const std::vector<Frame *> &frames, size_t cells, std::vector<int32_t> &slot);

// the arrays of a point set: per point the position, the mean viewing direction, dmax and the 32 descriptor bytes of Matcher::PointAttributes;
// as a struct of the library's own, and on a public Search struct (StereoTracker, StereoMapper), whose fields carry these names
bool append_point(MapPoint *mp, std::vector<MapPoint *> &points, std::vector<double> &pw, std::vector<double> &normal, std::vector<double> &dmax,
                  std::vector<uint8_t> &desc);
struct PointArrays {
    std::vector<MapPoint *> points;
    std::vector<double> pw, normal, dmax;
    std::vector<uint8_t> desc;
    bool append(MapPoint *mp) { return append_point(mp, points, pw, normal, dmax, desc); }     // false: refused, nothing appended
};
template <class Set> bool append_point(Set &s, MapPoint *mp) { return append_point(mp, s.points, s.pw, s.normal, s.dmax, s.desc); }

// a frame's keypoints: _pixel, _level (below 0 counts as 0) and the 32 descriptor bytes.  false at a null feature or one without 32 bytes
bool keypoint_arrays(const Frame *f, std::vector<double> &px, std::vector<int32_t> &level, std::vector<uint8_t> &desc);

// a pose optimisation's verdict on feature ft of frame f, as ba::OptimizeCurrentPoseOnly leaves it: _bad for an outlier; for an inlier also
// _depth, the z of its map point under f->_TCW (the new pose).  Returns whether ft is an inlier
bool apply_verdict(const Frame *f, Feature *ft, bool outlier);
}
}
#endif
