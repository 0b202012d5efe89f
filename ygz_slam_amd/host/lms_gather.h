// What ygz::LocalMapSelector (ygz_lms.cpp) and ygz::LocalMapTracker (ygz_lmt.cpp) share: the gather of the object graph into the flat arrays
// of the local-map selection (the keyframes by _keyframe_id, the points in the order they are met, the observations
// with their feature indices) and the one place that makes the device call.  Private to libygz_host.so like surface_share.h.  Pointer-keyed
// tables only answer "have I seen this object": every order goes by index, list position or id, never by address.
#ifndef YGZ_HOST_LMS_GATHER_H_
#define YGZ_HOST_LMS_GATHER_H_
#include "ygz/Basic.h"
#include "surface_share.h"
#include <algorithm>
#include <unordered_map>
namespace ygz {
namespace hip {

struct LmsGather {
    std::vector<Frame *> kfs;                                      // the keyframes of the call, ascending _keyframe_id
    std::vector<MapPoint *> pts;                                   // the points of the call, in the order they are met
    std::vector<uint8_t> kf_bad;
    std::vector<int32_t> cov, fr_off, fr_pt, offsets, obs_kf, obs_feat;
    size_t K = 1, C = 0, P = 1;                                    // the call's counts (at least one keyframe and one point)
    bool no_keyframe = true, no_point = true;
    int dropped = 0, observations = 0;

    static Frame *frame_of(unsigned long id, const Feature *f) { return f && f->_frame ? f->_frame : Memory::GetKeyFrame(id); }

    // steps 1 and 2 of LocalMapSelector::Select's header comment; every frame is non-null
    void gather(const std::vector<Frame *> &frames, int neighbours)
    {
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
            for (size_t j = 0; j < kf->_cov_keyframes.size() && j < (size_t)neighbours; ++j) meet(kf->_cov_keyframes[j]);
        }
        build(frames, neighbours, kf_at);
    }

    // the map of a list of keyframes alone, without a tracked frame (ygz::ResidentMap::Upload): the same rules on the keyframes as given,
    // null and repeated entries skipped; the points are those on the keyframes' features
    void gather_map(const std::vector<Frame *> &keyframes, int neighbours)
    {
        std::unordered_map<const Frame *, int32_t> kf_at;
        for (Frame *kf : keyframes)
            if (kf && kf_at.emplace(kf, 0).second) kfs.push_back(kf);
        build(std::vector<Frame *>(), neighbours, kf_at);
    }

    // step 2 on the keyframes met so far: their order, the covisible rows, the points and the observations
    void build(const std::vector<Frame *> &frames, int neighbours, std::unordered_map<const Frame *, int32_t> &kf_at)
    {
        std::stable_sort(kfs.begin(), kfs.end(), [](const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; });
        for (size_t k = 0; k < kfs.size(); ++k) kf_at[kfs[k]] = (int32_t)k;
        no_keyframe = kfs.empty();                                 // no frame has a point with an observer: every list is empty
        K = std::max<size_t>(kfs.size(), 1); C = (size_t)neighbours;
        kf_bad.assign(K, 0);
        cov.assign(K * C, -1);
        std::unordered_map<const Feature *, int32_t> feat_at;      // a feature of a keyframe of the call -> its index there
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
        // the points, in the order they are met: on the frames, then on the keyframes
        std::unordered_map<const MapPoint *, int32_t> pt_at;
        const auto point = [&](MapPoint *mp) { const auto r = pt_at.emplace(mp, (int32_t)pts.size()); if (r.second) pts.push_back(mp); return r.first->second; };
        fr_off.assign(1, 0);
        for (const Frame *f : frames) {
            for (const Feature *ft : f->_features) fr_pt.push_back(ft && good(ft->_mappoint) ? point(ft->_mappoint) : -1);
            fr_off.push_back((int32_t)fr_pt.size());
        }
        for (const Frame *kf : kfs)
            for (const Feature *ft : kf->_features)
                if (ft && good(ft->_mappoint)) point(ft->_mappoint);
        no_point = pts.empty();
        offsets.assign(1, 0);
        std::vector<std::pair<int32_t, int32_t>> row;
        for (const MapPoint *mp : pts) {
            row.clear();
            for (const auto &ob : mp->_obs) {
                const auto k = kf_at.find(frame_of(ob.first, ob.second));
                if (k == kf_at.end()) continue;                    // a keyframe that is no part of this call
                const auto j = feat_at.find(ob.second);
                const Frame *kf = kfs[(size_t)k->second];
                if (!ob.second || j == feat_at.end() || ob.second->_mappoint != mp || (size_t)j->second >= kf->_features.size() ||
                    kf->_features[(size_t)j->second] != ob.second) { ++dropped; continue; }
                row.emplace_back(k->second, j->second);
            }
            std::stable_sort(row.begin(), row.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first < b.first; });
            for (size_t i = 0; i < row.size(); ++i) {
                if (i && row[i].first == row[i - 1].first) { ++dropped; continue; }
                obs_kf.push_back(row[i].first); obs_feat.push_back(row[i].second);
            }
            offsets.push_back((int32_t)obs_kf.size());
        }
        if (no_point) offsets.push_back(0);                        // the call wants a point: one without observations
        P = offsets.size() - 1;
        observations = (int)obs_kf.size();
        if (obs_kf.empty()) { obs_kf.push_back(0); obs_feat.push_back(0); }
        if (fr_pt.empty()) fr_pt.push_back(-1);
        if (cov.empty()) cov.push_back(-1);
    }
};

// what the selection answered: per frame ref, n_voters, n_local, n_pt, n_cut; local_kf [F][K]; local_pt [F][MP]; prior by frame entry
struct LmsAnswer {
    size_t MP = 0;
    std::vector<int32_t> ref, n_voters, n_local, local_kf, n_pt, n_cut, local_pt, prior;
};

// the ONE call of the local-map selection on a gather of F frames (ygz_lms.cpp); max_points is cut to the points of the call.  false: logged
// under `who`
bool lms_select(const char *who, const LmsGather &g, size_t F, int max_keyframes, int max_points, LmsAnswer &a);

}
}
#endif
