// ygz::StereoRefTracker (include/ygz/Algorithm/StereoRefTracker.h): nothing in the reference.  ORB-SLAM2's TrackReferenceKeyFrame for any number
// of frames: the point sets of the reference keyframes are built on the host, the frames' and keyframes' feature lists and depths are put into
// their slots (hip::load_slots, surface_share.h), then ONE entry point (ygz_hip_stereo_ref_keyframe_slots, ygz_slam_amd/csrc/srk.hip) computes the BoW
// of every slot, searches, claims, removes by orientation and optimises on the device, and the frames are edited from its result in frame
// order.  The spec is DESIGN.md section 29.  Every order goes by index or list position, never by address.  Error conventions of the other
// surfaces: a failed call logs and returns 0, only a missing device throws.
#include "ygz/Algorithm/StereoRefTracker.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include <algorithm>
#include <map>

namespace ygz {

namespace {
using hip::good;

struct PointSet {
    std::vector<MapPoint *> points;
    std::vector<double> pw;
};
}

int StereoRefTracker::TrackReferenceKeyFrame(const std::vector<Frame *> &frames, const std::vector<Frame *> &reference_keyframes,
                                             std::vector<Result> *results)
{
    if (results) results->clear();
    const size_t n = frames.size();
    if (n == 0 || reference_keyframes.size() != n || !Frame::GetCamera()) {
        LOG(ERROR) << "StereoRefTracker::TrackReferenceKeyFrame: no frame, no camera, or keyframes of another length" << endl;
        return 0;
    }
    hip::Runtime &rt = hip::Runtime::Get();
    ygz_hip_ctx *c = rt.ctx();
    const size_t cells = (size_t)rt.cells();
    // 1: the distinct keyframes in the order they first appear, one set each
    std::vector<Frame *> kfs;
    std::vector<int32_t> kf_of(n);
    for (size_t k = 0; k < n; ++k) {
        if (!frames[k] || !reference_keyframes[k] || frames[k] == reference_keyframes[k] ||
            std::find(frames.begin(), frames.begin() + (long)k, frames[k]) != frames.begin() + (long)k) {
            LOG(ERROR) << "StereoRefTracker::TrackReferenceKeyFrame: a null or repeated frame, no keyframe, or a frame that is its own keyframe" << endl;
            return 0;
        }
        const auto it = std::find(kfs.begin(), kfs.end(), reference_keyframes[k]);
        kf_of[k] = (int32_t)(it - kfs.begin());
        if (it == kfs.end()) kfs.push_back(reference_keyframes[k]);
    }
    std::vector<Frame *> all(kfs);                                       // every frame that needs a slot, keyframes first, each once
    for (Frame *f : frames)
        if (std::find(all.begin(), all.end(), f) == all.end()) all.push_back(f);
    if (!hip::loadable("StereoRefTracker::TrackReferenceKeyFrame", all, cells)) return 0;      // before kf_point is indexed by feature
    std::vector<PointSet> sets(kfs.size());
    std::vector<ygz_strack_points> views(kfs.size());
    std::vector<int32_t> kf_point(kfs.size() * cells, -1), kf_set(kfs.size());
    for (size_t s = 0; s < kfs.size(); ++s) {
        std::map<const MapPoint *, int32_t> index;
        for (size_t i = 0; i < kfs[s]->_features.size(); ++i) {
            const Feature *ft = kfs[s]->_features[i];
            if (!good(ft->_mappoint)) continue;
            const auto at = index.find(ft->_mappoint);
            if (at != index.end()) { kf_point[s * cells + i] = at->second; continue; }
            index[ft->_mappoint] = kf_point[s * cells + i] = (int32_t)sets[s].points.size();
            sets[s].points.push_back(ft->_mappoint);
            for (int k = 0; k < 3; ++k) sets[s].pw.push_back(ft->_mappoint->_pos_world[k]);
        }
        ygz_strack_points &v = views[s];
        v.pw = sets[s].pw.data(); v.pt_desc = nullptr; v.pt_level = nullptr; v.pt_angle = nullptr; v.pt_dmax = nullptr; v.pt_normal = nullptr;
        v.n_pt = (int)sets[s].points.size();
        kf_set[s] = (int32_t)s;
    }
    // 2: the frames into their slots, with their feature lists and depths
    std::vector<int32_t> all_slot;
    if (!hip::load_slots("StereoRefTracker::TrackReferenceKeyFrame", all, cells, all_slot)) return 0;
    // 3: one call
    const std::vector<int32_t> kf_slot(all_slot.begin(), all_slot.begin() + (long)kfs.size());       // `all` begins with the keyframes
    std::vector<int32_t> slot(n), status(n), counts(8 * n), kp_point(n * cells), inliers(n);
    std::vector<uint8_t> outlier(n * cells);
    std::vector<double> T(7 * n), T_out(7 * n);
    for (size_t k = 0; k < n; ++k) { slot[k] = all_slot[(size_t)(std::find(all.begin(), all.end(), frames[k]) - all.begin())]; frames[k]->_TCW.to7(&T[7 * k]); }
    ygz_srk_params prm;
    ygz_hip_default_srk_params(&prm);
    prm.baseline = _options._baseline; prm.th_low = _options._th_low; prm.knn_ratio = _options._knn_ratio; prm.levelsup = _options._levelsup;
    prm.check_orientation = _options._check_orientation ? 1 : 0; prm.min_matches = _options._min_matches; prm.min_inliers = _options._min_inliers;
    if (!hip::check(ygz_hip_stereo_ref_keyframe_slots(c, (int)views.size(), views.data(), (int)kfs.size(), kf_slot.data(), kf_set.data(),
                                                      kf_point.data(), (int)n, slot.data(), kf_of.data(), T.data(), &prm, T_out.data(),
                                                      status.data(), counts.data(), kp_point.data(), nullptr, outlier.data(), nullptr,
                                                      inliers.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                      nullptr), "stereo_ref_keyframe_slots"))
        return 0;
    // 4: the frames, in frame order
    int tracked = 0;
    if (results) results->resize(n);
    for (size_t k = 0; k < n; ++k) {
        Frame *f = frames[k];
        const PointSet &s = sets[(size_t)kf_of[k]];
        const int32_t *kp = &kp_point[k * cells];
        for (Feature *ft : f->_features) ft->_mappoint = nullptr;
        int kept = 0;
        if (status[k] != 1) {
            for (size_t j = 0; j < f->_features.size(); ++j)
                if (kp[j] >= 0 && (size_t)kp[j] < s.points.size()) f->_features[j]->_mappoint = s.points[(size_t)kp[j]];
            f->_TCW = SE3::from7(&T_out[7 * k]);
            for (size_t j = 0; j < f->_features.size(); ++j) {
                Feature *ft = f->_features[j];
                if (!good(ft->_mappoint)) continue;
                if (!hip::apply_verdict(f, ft, outlier[k * cells + j] != 0)) ft->_mappoint = nullptr;
                else if (!ft->_mappoint->_obs.empty()) ++kept;
            }
        }
        const bool ok = status[k] == 0 && kept >= _options._min_tracked;
        if (ok) ++tracked;
        if (!results) continue;
        Result &r = (*results)[k];
        r.status = status[k]; r.matches = status[k] == 1 ? 0 : counts[8 * k + 7]; r.inliers = inliers[k]; r.kept = kept; r.tracked = ok;
    }
    return tracked;
}

}  // namespace ygz
