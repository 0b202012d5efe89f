// ygz::StereoLocalMap (include/ygz/Algorithm/StereoLocalMap.h): nothing in the reference.  ORB-SLAM2's TrackLocalMap for any number of frames:
// the point sets of the local keyframe lists are built on the host, the frames' feature lists and depths are put into their slots
// (hip::load_slots, surface_share.h), then ONE entry point (ygz_hip_stereo_local_map_slots, ygz_slam_amd/csrc/slm.hip) searches, claims and
// optimises on the device, and the frames and map points are edited from its result in frame order.  The spec is DESIGN.md section 28.
// Every order goes by index or list position, never by address.  Error conventions of the other surfaces: a failed call logs and returns
// 0, only a missing device throws.
#include "ygz/Algorithm/StereoLocalMap.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include <algorithm>
#include <map>
#include <set>

namespace ygz {

namespace {
using hip::good;

struct PointSet : hip::PointArrays { std::map<const MapPoint *, int32_t> index; };      // a point of the set -> its position

void build_set(const std::vector<Frame *> &keyframes, PointSet &s)
{
    std::set<const MapPoint *> seen;
    for (const Frame *kf : keyframes) {
        if (!kf) continue;
        for (const Feature *f : kf->_features)
            if (f && good(f->_mappoint) && seen.insert(f->_mappoint).second && s.append(f->_mappoint)) s.index[f->_mappoint] = (int32_t)s.points.size() - 1;
    }
}
}

int StereoLocalMap::TrackLocalMap(const std::vector<Frame *> &frames, const std::vector<const std::vector<Frame *> *> &local_keyframes,
                                  std::vector<Result> *results)
{
    if (results) results->clear();
    const size_t n = frames.size();
    if (n == 0 || local_keyframes.size() != n || !Frame::GetCamera()) {
        LOG(ERROR) << "StereoLocalMap::TrackLocalMap: no frame, no camera, or keyframe lists of another length" << endl;
        return 0;
    }
    hip::Runtime &rt = hip::Runtime::Get();
    ygz_hip_ctx *c = rt.ctx();
    const size_t cells = (size_t)rt.cells();
    for (size_t k = 0; k < n; ++k)
        if (!frames[k] || !local_keyframes[k] || std::find(frames.begin(), frames.begin() + (long)k, frames[k]) != frames.begin() + (long)k) {
            LOG(ERROR) << "StereoLocalMap::TrackLocalMap: a null or repeated frame, or a frame without a keyframe list" << endl;
            return 0;
        }
    if (!hip::loadable("StereoLocalMap::TrackLocalMap", frames, cells)) return 0;      // before prior is indexed by feature
    // 1: one set per distinct list object, in the order the lists first appear
    std::vector<const std::vector<Frame *> *> lists;
    std::vector<int32_t> set_of(n);
    for (size_t k = 0; k < n; ++k) {
        const auto it = std::find(lists.begin(), lists.end(), local_keyframes[k]);
        set_of[k] = (int32_t)(it - lists.begin());
        if (it == lists.end()) lists.push_back(local_keyframes[k]);
    }
    std::vector<PointSet> sets(lists.size());
    std::vector<ygz_strack_points> views(lists.size());
    for (size_t s = 0; s < lists.size(); ++s) {
        build_set(*lists[s], sets[s]);
        ygz_strack_points &v = views[s];
        v.pw = sets[s].pw.data(); v.pt_desc = sets[s].desc.data(); v.pt_level = nullptr; v.pt_angle = nullptr;
        v.pt_dmax = sets[s].dmax.data(); v.pt_normal = sets[s].normal.data(); v.n_pt = (int)sets[s].points.size();
    }
    // the associations the frames come with
    std::vector<int32_t> prior(n * cells, -1);
    for (size_t k = 0; k < n; ++k) {
        const PointSet &s = sets[(size_t)set_of[k]];
        for (size_t j = 0; j < frames[k]->_features.size(); ++j) {
            const Feature *ft = frames[k]->_features[j];
            if (!good(ft->_mappoint)) continue;
            const auto it = s.index.find(ft->_mappoint);
            if (it == s.index.end()) {
                LOG(ERROR) << "StereoLocalMap::TrackLocalMap: a map point on a frame that is not among its local keyframes' points" << endl;
                return 0;
            }
            prior[k * cells + j] = it->second;
        }
    }
    // 2: the frames into their slots, with their feature lists and depths
    std::vector<int32_t> slot;
    if (!hip::load_slots("StereoLocalMap::TrackLocalMap", frames, cells, slot)) return 0;
    // 3: one call
    size_t pairs = 0;
    std::vector<size_t> off(n + 1, 0);
    for (size_t k = 0; k < n; ++k) { pairs += sets[(size_t)set_of[k]].points.size(); off[k + 1] = pairs; }
    std::vector<double> T(7 * n), T_out(7 * n);
    for (size_t k = 0; k < n; ++k) frames[k]->_TCW.to7(&T[7 * k]);
    std::vector<int32_t> status(n), counts(8 * n), kp_point(n * cells), inliers(n), reason(pairs + 1);
    std::vector<uint8_t> outlier(n * cells);
    ygz_slm_params prm;
    ygz_hip_default_slm_params(&prm);
    prm.baseline = _options._baseline; prm.th = _options._th; prm.ratio = _options._ratio; prm.r_near = _options._r_near;
    prm.r_wide = _options._r_wide; prm.cos_near = _options._cos_near; prm.th_dist = _options._th_dist; prm.min_edges = _options._min_edges;
    if (!hip::check(ygz_hip_stereo_local_map_slots(c, (int)views.size(), views.data(), (int)n, slot.data(), set_of.data(), T.data(), prior.data(),
                                                   &prm, T_out.data(), status.data(), counts.data(), kp_point.data(), outlier.data(), nullptr,
                                                   inliers.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                   reason.data(), nullptr, nullptr, nullptr, nullptr), "stereo_local_map_slots"))
        return 0;
    // 4: the frames and the map points, in frame order
    int tracked = 0;
    if (results) results->resize(n);
    for (size_t k = 0; k < n; ++k) {
        Frame *f = frames[k];
        const PointSet &s = sets[(size_t)set_of[k]];
        const int32_t *pr = &prior[k * cells], *kp = &kp_point[k * cells];
        std::set<const MapPoint *> on_frame;
        for (size_t j = 0; j < f->_features.size(); ++j)
            if (pr[j] >= 0 && on_frame.insert(s.points[(size_t)pr[j]]).second) ++s.points[(size_t)pr[j]]->_cnt_visible;
        for (size_t i = 0; i < s.points.size(); ++i) {
            MapPoint *mp = s.points[i];
            if (on_frame.count(mp)) continue;                            // skipped through the prior: not touched
            if (reason[off[k] + i] == 0) { ++mp->_cnt_visible; mp->_track_in_view = true; }
            else mp->_track_in_view = false;
        }
        for (size_t j = 0; j < f->_features.size(); ++j)
            if (pr[j] < 0 && kp[j] >= 0 && (size_t)kp[j] < s.points.size()) f->_features[j]->_mappoint = s.points[(size_t)kp[j]];
        f->_TCW = SE3::from7(&T_out[7 * k]);
        for (size_t j = 0; j < f->_features.size(); ++j) {
            Feature *ft = f->_features[j];
            if (kp[j] < 0 || !good(ft->_mappoint)) continue;
            if (hip::apply_verdict(f, ft, outlier[k * cells + j] != 0)) ft->_mappoint->_cnt_found++;
        }
        const bool ok = status[k] == 0 && inliers[k] >= _options._min_tracked;
        if (ok) ++tracked;
        if (!results) continue;
        Result &r = (*results)[k];
        r.status = status[k]; r.new_matches = counts[8 * k + 6]; r.edges = counts[8 * k + 7]; r.inliers = inliers[k]; r.tracked = ok;
    }
    return tracked;
}

}  // namespace ygz
