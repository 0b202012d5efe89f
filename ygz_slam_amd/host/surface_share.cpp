// surface_share.h: what the class surfaces share.  The spec is DESIGN.md section 31.
#include "surface_share.h"
#include "ygz/Algorithm/Matcher.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <algorithm>
#include <cstring>

namespace ygz {
namespace hip {

FeatureArrays::FeatureArrays(const Frame *f)
{
    for (const Feature *ft : f->_features) {
        px.push_back(ft->_pixel[0]); px.push_back(ft->_pixel[1]);
        level.push_back(std::max(ft->_level, 0));
        angle.push_back((float)ft->_angle);
        depth.push_back(ft->_depth);
        has.push_back(ft->_depth > 0 ? 1 : 0);
    }
}

bool loadable(const char *who, const std::vector<Frame *> &frames, size_t cells)
{
    for (const Frame *f : frames) {
        if (!f) { LOG(ERROR) << who << ": a null frame" << endl; return false; }
        if (f->_features.size() > cells) { LOG(ERROR) << who << ": a frame with more features than the context has cells" << endl; return false; }
        for (const Feature *ft : f->_features)
            if (!ft) { LOG(ERROR) << who << ": a null feature" << endl; return false; }
    }
    return true;
}

bool load_slots(const char *who, const std::vector<Frame *> &frames, size_t cells, std::vector<int32_t> &slot)
{
    if (!loadable(who, frames, cells)) return false;
    Runtime &rt = Runtime::Get();
    ygz_hip_ctx *c = rt.ctx();
    slot.resize(frames.size());
    for (size_t k = 0; k < frames.size(); ++k) slot[k] = rt.Resident(frames[k]);
    for (size_t k = 0; k < frames.size(); ++k)                           // a later frame may have taken an earlier one's slot
        if (slot[k] < 0 || rt.Resident(frames[k]) != slot[k]) { LOG(ERROR) << who << ": more distinct frames than the runtime keeps resident" << endl; return false; }
    for (size_t k = 0; k < frames.size(); ++k) {
        const FeatureArrays a(frames[k]);
        const int m = (int)a.level.size();
        if (!check(ygz_hip_describe_given_angle(c, slot[k], a.px.data(), a.level.data(), a.angle.data(), m), "describe_given_angle")) return false;
        if (!check(ygz_hip_set_keypoint_depths(c, slot[k], a.depth.data(), a.has.data(), m), "set_keypoint_depths")) return false;
    }
    return true;
}

bool append_point(MapPoint *mp, std::vector<MapPoint *> &points, std::vector<double> &pw, std::vector<double> &normal, std::vector<double> &dmax,
                  std::vector<uint8_t> &desc)
{
    Matcher::PointAttr a;
    if (!Matcher::PointAttributes(mp, a)) return false;
    points.push_back(mp);
    for (int k = 0; k < 3; ++k) { pw.push_back(mp->_pos_world[k]); normal.push_back(a.normal[k]); }
    dmax.push_back(a.dmax);
    desc.insert(desc.end(), a.desc, a.desc + 32);
    return true;
}

bool keypoint_arrays(const Frame *f, std::vector<double> &px, std::vector<int32_t> &level, std::vector<uint8_t> &desc)
{
    const size_t n = f->_features.size();
    px.resize(2 * n); level.resize(n); desc.resize(32 * n);
    for (size_t i = 0; i < n; ++i) {
        const Feature *ft = f->_features[i];
        if (!ft || !ft->_desc.data || ft->_desc.rows * ft->_desc.cols * (int)ft->_desc.elemSize() < 32) return false;
        px[2 * i] = ft->_pixel[0]; px[2 * i + 1] = ft->_pixel[1];
        level[i] = std::max(ft->_level, 0);
        memcpy(&desc[32 * i], ft->_desc.data, 32);
    }
    return true;
}

bool apply_verdict(const Frame *f, Feature *ft, bool outlier)
{
    ft->_bad = outlier;
    if (!outlier) ft->_depth = Frame::_camera->World2Camera(ft->_mappoint->_pos_world, f->_TCW)[2];
    return !outlier;
}

}  // namespace hip
}  // namespace ygz
