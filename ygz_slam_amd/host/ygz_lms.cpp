// ygz::LocalMapSelector (include/ygz/Algorithm/LocalMapSelector.h): nothing in the reference.  StereoTracker::LocalKeyFrames and the point set
// of StereoLocalMap::TrackLocalMap for any number of frames through ONE entry point (ygz_hip_local_map_select, ygz_slam_amd/csrc/lms.hip).  The
// host gathers the object graph into the flat arrays of the call -- the keyframes by _keyframe_id, the points in the order they are met, the
// observations with their feature indices -- and turns the answer back into lists.  The spec is DESIGN.md section 34.  Pointer-keyed tables
// only answer "have I seen this object": every order goes by index, list position or id, never by address.  Error conventions of the other
// surfaces: a failed call logs and returns 0, only a missing device throws.
#include "ygz/Algorithm/LocalMapSelector.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include <algorithm>
#include <map>
#include <unordered_map>

namespace ygz {

namespace {
using hip::good;
Frame *frame_of(unsigned long id, const Feature *f) { return f && f->_frame ? f->_frame : Memory::GetKeyFrame(id); }
}

int LocalMapSelector::Select(const std::vector<Frame *> &frames, std::vector<Result> *results)
{
    if (results) results->clear();
    _keyframe_lists.clear();
    _point_lists.clear();
    _stats = Stats();
    if (frames.empty()) { LOG(ERROR) << "LocalMapSelector::Select: no frame" << endl; return 0; }
    for (const Frame *f : frames)
        if (!f) { LOG(ERROR) << "LocalMapSelector::Select: a null frame" << endl; return 0; }
    if (_options._neighbours < 0) { LOG(ERROR) << "LocalMapSelector::Select: _neighbours below 0" << endl; return 0; }
    // 1: the keyframes, in the order they are met, then by id
    std::vector<Frame *> kfs;
    std::unordered_map<const Frame *, int32_t> kf_at;
    const auto meet = [&](Frame *kf) { if (kf && kf_at.emplace(kf, 0).second) kfs.push_back(kf); };
    for (const Frame *f : frames)
        for (const Feature *ft : f->_features) {
            if (!ft || !good(ft->_mappoint)) continue;
            for (const auto &ob : ft->_mappoint->_obs) meet(frame_of(ob.first, ob.second));
        }
    const size_t observers = kfs.size();
    for (size_t i = 0; i < observers; ++i) {
        const Frame *kf = kfs[i];
        for (size_t j = 0; j < kf->_cov_keyframes.size() && j < (size_t)_options._neighbours; ++j) meet(kf->_cov_keyframes[j]);
    }
    std::stable_sort(kfs.begin(), kfs.end(), [](const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; });
    for (size_t k = 0; k < kfs.size(); ++k) kf_at[kfs[k]] = (int32_t)k;
    const bool no_keyframe = kfs.empty();                          // no frame has a point with an observer: every list is empty
    const size_t K = std::max<size_t>(kfs.size(), 1), C = (size_t)_options._neighbours;
    std::vector<uint8_t> kf_bad(K, 0);
    std::vector<int32_t> cov(K * C, -1);
    std::unordered_map<const Feature *, int32_t> feat_at;          // a feature of a keyframe of the call -> its index there
    for (size_t k = 0; k < kfs.size(); ++k) {
        const Frame *kf = kfs[k];
        kf_bad[k] = kf->_bad ? 1 : 0;
        for (size_t j = 0; j < kf->_cov_keyframes.size() && j < C; ++j) {
            const auto it = kf_at.find(kf->_cov_keyframes[j]);
            if (kf->_cov_keyframes[j] && it != kf_at.end()) cov[k * C + j] = it->second;
        }
        for (size_t j = 0; j < kf->_features.size(); ++j)
            if (kf->_features[j]) feat_at.emplace(kf->_features[j], (int32_t)j);
    }
    // 2: the points, in the order they are met: on the frames, then on the keyframes
    std::vector<MapPoint *> pts;
    std::unordered_map<const MapPoint *, int32_t> pt_at;
    const auto point = [&](MapPoint *mp) { const auto r = pt_at.emplace(mp, (int32_t)pts.size()); if (r.second) pts.push_back(mp); return r.first->second; };
    std::vector<int32_t> fr_off(1, 0), fr_pt;
    for (const Frame *f : frames) {
        for (const Feature *ft : f->_features) fr_pt.push_back(ft && good(ft->_mappoint) ? point(ft->_mappoint) : -1);
        fr_off.push_back((int32_t)fr_pt.size());
    }
    for (const Frame *kf : kfs)
        for (const Feature *ft : kf->_features)
            if (ft && good(ft->_mappoint)) point(ft->_mappoint);
    const bool no_point = pts.empty();
    std::vector<int32_t> offsets(1, 0), obs_kf, obs_feat;
    std::vector<std::pair<int32_t, int32_t>> row;
    for (const MapPoint *mp : pts) {
        row.clear();
        for (const auto &ob : mp->_obs) {
            const auto k = kf_at.find(frame_of(ob.first, ob.second));
            if (k == kf_at.end()) continue;                        // a keyframe that is no part of this call
            const auto j = feat_at.find(ob.second);
            const Frame *kf = kfs[(size_t)k->second];
            if (!ob.second || j == feat_at.end() || ob.second->_mappoint != mp || (size_t)j->second >= kf->_features.size() ||
                kf->_features[(size_t)j->second] != ob.second) { ++_stats.dropped; continue; }
            row.emplace_back(k->second, j->second);
        }
        std::stable_sort(row.begin(), row.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first < b.first; });
        for (size_t i = 0; i < row.size(); ++i) {
            if (i && row[i].first == row[i - 1].first) { ++_stats.dropped; continue; }
            obs_kf.push_back(row[i].first); obs_feat.push_back(row[i].second);
        }
        offsets.push_back((int32_t)obs_kf.size());
    }
    if (no_point) offsets.push_back(0);                            // the call wants a point: one without observations
    const size_t P = offsets.size() - 1, F = frames.size();
    _stats.frames = (int)F; _stats.keyframes = (int)kfs.size(); _stats.points = (int)pts.size(); _stats.observations = (int)obs_kf.size();
    if (obs_kf.empty()) { obs_kf.push_back(0); obs_feat.push_back(0); }
    if (fr_pt.empty()) fr_pt.push_back(-1);
    if (cov.empty()) cov.push_back(-1);
    // 3
    ygz_lms_params prm;
    ygz_hip_default_lms_params(&prm);
    prm.max_keyframes = _options._local_keyframes_max;
    prm.max_points = std::min<int64_t>(_options._max_points, (int64_t)P);       // no set is larger than the points of the call
    if (prm.max_points < 1) { LOG(ERROR) << "LocalMapSelector::Select: _max_points below 1" << endl; return 0; }
    const size_t MP = (size_t)prm.max_points, E = (size_t)fr_off.back();
    std::vector<int32_t> ref(F), n_voters(F), n_local(F), local_kf(F * K), n_pt(F), n_cut(F), local_pt(F * MP), prior(std::max<size_t>(E, 1));
    if (!hip::check(ygz_hip_local_map_select(hip::Runtime::Get().ctx(), (int)K, kf_bad.data(), (int)C, cov.data(), (int)P, offsets.data(), obs_kf.data(),
                                             obs_feat.data(), nullptr, (int)F, fr_off.data(), fr_pt.data(), &prm, nullptr, ref.data(),
                                             n_voters.data(), n_local.data(), local_kf.data(), n_pt.data(), n_cut.data(), local_pt.data(),
                                             prior.data()), "local_map_select")) return 0;
    // 4: equal lists share one object
    std::map<std::vector<int32_t>, size_t> seen;
    int with_list = 0;
    for (size_t f = 0; f < F; ++f) {
        const int32_t *lk = local_kf.data() + f * K, *lp = local_pt.data() + f * MP;
        const std::vector<int32_t> key(lk, lk + (no_keyframe ? 0 : n_local[f]));
        const auto at = seen.emplace(key, _keyframe_lists.size());
        if (at.second) {
            _keyframe_lists.emplace_back(new std::vector<Frame *>());
            _point_lists.emplace_back(new std::vector<MapPoint *>());
            for (int32_t k : key) _keyframe_lists.back()->push_back(kfs[(size_t)k]);
            for (int i = 0; i < n_pt[f] && !key.empty(); ++i) _point_lists.back()->push_back(pts[(size_t)lp[i]]);
        }
        Frame *best = !no_keyframe && ref[f] >= 0 ? kfs[(size_t)ref[f]] : nullptr;
        if (best) frames[f]->_ref_keyframe = best;
        if (!key.empty()) ++with_list;
        if (!results) continue;
        Result r;
        r.keyframes = _keyframe_lists[at.first->second].get();
        r.points = _point_lists[at.first->second].get();
        r.prior.assign(prior.begin() + fr_off[f], prior.begin() + fr_off[f + 1]);
        r.ref = best; r.voters = n_voters[f]; r.cut = n_cut[f];
        results->push_back(r);
    }
    _stats.lists = (int)_keyframe_lists.size();
    return with_list;
}

}  // namespace ygz
