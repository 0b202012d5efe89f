// ygz::StereoMatcher (include/ygz/Algorithm/StereoMatcher.h) over ygz_hip_stereo_match: the features of the two frames as the ABI's arrays, the
// pictures from the frames' HBM slots, one device call (ygz_slam_amd/csrc/stereo.hip).  Error conventions of the other surfaces: a failed call
// logs and returns 0, only a missing device throws.
#include "ygz/Algorithm/StereoMatcher.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <cstring>

namespace ygz {

namespace {
struct Arrays { vector<double> px; vector<int32_t> level; vector<uint8_t> desc; };
// false when a feature is null or has no 32-byte descriptor
bool gather(const Frame *f, Arrays &a)
{
    const size_t n = f->_features.size();
    a.px.resize(2 * n); a.level.resize(n); a.desc.resize(32 * n);
    for (size_t i = 0; i < n; ++i) {
        const Feature *ft = f->_features[i];
        if (!ft || ft->_desc.empty() || (size_t)ft->_desc.cols * ft->_desc.elemSize() < 32) return false;
        a.px[2 * i] = ft->_pixel[0]; a.px[2 * i + 1] = ft->_pixel[1];
        a.level[i] = ft->_level;
        memcpy(&a.desc[32 * i], ft->_desc.data, 32);
    }
    return true;
}
}

int StereoMatcher::ComputeStereoMatches(Frame *left, Frame *right, std::vector<double> *u_right)
{
    _status.clear();
    if (u_right) u_right->clear();
    if (!left || !right || left == right) { LOG(ERROR) << "StereoMatcher::ComputeStereoMatches: two different frames are needed" << endl; return 0; }
    Arrays a, b;
    if (!gather(left, a) || !gather(right, b)) { LOG(ERROR) << "StereoMatcher::ComputeStereoMatches: a feature without a descriptor" << endl; return 0; }
    const int nl = (int)left->_features.size(), nr = (int)right->_features.size();
    _status.assign((size_t)nl, YGZ_STEREO_NO_CANDIDATE);
    if (u_right) u_right->assign((size_t)nl, -1.0);
    if (nl == 0) return 0;
    hip::Runtime &rt = hip::Runtime::Get();
    const int sl = rt.Resident(left), sr = rt.Resident(right);
    if (sl < 0 || sr < 0 || left->_hip_slot != sl) {              // the second upload took the first frame's slot: fewer than two slots
        LOG(ERROR) << "StereoMatcher::ComputeStereoMatches: the two frames are not resident together" << endl;
        return 0;
    }
    ygz_stereo_params p;
    ygz_hip_default_stereo_params(&p);
    p.baseline = _options._baseline; p.min_disparity = _options._min_disparity; p.max_disparity = _options._max_disparity;
    p.th_dist = _options._th_dist; p.write_depths = 0;
    vector<double> depth((size_t)nl), ur((size_t)nl);
    vector<int32_t> status((size_t)nl);
    if (!hip::check(ygz_hip_stereo_match(rt.ctx(), sl, sr, a.px.data(), a.level.data(), a.desc.data(), nl, b.px.data(), b.level.data(), b.desc.data(), nr,
                                         &p, nullptr, ur.data(), depth.data(), nullptr, status.data(), nullptr), "stereo_match")) return 0;
    int set = 0;
    for (int i = 0; i < nl; ++i) {
        _status[i] = status[i];
        if (status[i] != YGZ_STEREO_OK) continue;
        left->_features[i]->_depth = depth[i];
        if (u_right) (*u_right)[i] = ur[i];
        ++set;
    }
    return set;
}

}  // namespace ygz
