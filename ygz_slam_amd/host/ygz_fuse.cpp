// ygz::LoopClosing::FuseLoop / ReplaceMapPoint / UpdateCovisibility and Matcher::ComputeDistinctiveDescriptors (include/ygz/Algorithm/
// LoopClosing.h, Matcher.h): nothing in the reference.  The rest of ORB-SLAM2's LoopClosing::CorrectLoop up to the global BA (ygz_gba.cpp): the current
// keyframe's loop matches and the hits of Matcher::SearchFuseCandidates over the corrected neighbourhood are acted on (MapPoint::Replace /
// AddObservation on this data model), then the two pieces of map upkeep that forces run on the device, one call each:
// ygz_hip_distinctive_descriptors and ygz_hip_covisibility (ygz_slam_amd/csrc/map.hip).  Every order ORB-SLAM2 leaves to set iteration over
// pointers goes by keyframe id or index here.  Error conventions of the other surfaces: a failed call logs and returns 0 / false, only a
// missing device throws.
#include "ygz/Algorithm/LoopClosing.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include <algorithm>
#include <cstring>

namespace ygz {

namespace {
bool by_id(const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; }
using hip::good;

// not bad, once each, by id
vector<Frame *> universe_of(const vector<Frame *> &keyframes)
{
    vector<Frame *> u;
    for (Frame *k : keyframes) if (k && !k->_bad) u.push_back(k);
    std::sort(u.begin(), u.end(), by_id);
    u.erase(std::unique(u.begin(), u.end()), u.end());
    return u;
}

const int kCovisibilityTh = 15;                       // Frame::UpdateConnections' threshold
}

// ------------------------------------------------------------------------------------------ Matcher::ComputeDistinctiveDescriptors
int Matcher::ComputeDistinctiveDescriptors(const vector<MapPoint *> &points)
{
    vector<MapPoint *> pts;
    vector<int32_t> offsets(1, 0);
    vector<uint8_t> desc;
    int set = 0;
    // one device call per YGZ_MAP_MAX_OBS observations (a map of this project fits in one)
    auto flush = [&]() -> bool {
        if (pts.empty()) return true;
        vector<int32_t> best(pts.size());
        vector<uint8_t> out(32 * pts.size());
        const bool ok = hip::check(ygz_hip_distinctive_descriptors(hip::Runtime::Get().ctx(), (int)pts.size(), offsets.data(), desc.data(), best.data(),
                                                                   nullptr, out.data()), "distinctive_descriptors");
        for (size_t p = 0; ok && p < pts.size(); ++p) {
            Mat d(1, 32, CV_8UC1);
            memcpy(d.data, &out[32 * p], 32);
            pts[p]->_distinctive_desc = d;
            ++set;
        }
        pts.clear(); offsets.assign(1, 0); desc.clear();
        return ok;
    };
    for (MapPoint *mp : points) {
        if (!good(mp)) continue;
        size_t n = 0;
        const size_t first = desc.size();
        for (const auto &ob : mp->_obs) {                               // key order
            const Feature *f = ob.second;
            if (!f || !f->_desc.data || f->_desc.rows * f->_desc.cols * (int)f->_desc.elemSize() != 32
                || (f->_desc.rows > 1 && f->_desc.step != (size_t)f->_desc.cols * f->_desc.elemSize())) continue;
            desc.insert(desc.end(), f->_desc.data, f->_desc.data + 32);
            ++n;
        }
        if (n == 0 || n > YGZ_MAP_MAX_OBS_PER_POINT) { desc.resize(first); continue; }
        if (desc.size() / 32 > YGZ_MAP_MAX_OBS) {                       // this point opens the next call
            vector<uint8_t> own(desc.begin() + first, desc.end());
            desc.resize(first);
            if (!flush()) return set;
            desc = own;
        }
        pts.push_back(mp);
        offsets.push_back((int32_t)(desc.size() / 32));
    }
    flush();
    return set;
}

// ------------------------------------------------------------------------------------------ LoopClosing::ReplaceMapPoint
void LoopClosing::ReplaceMapPoint(MapPoint *from, MapPoint *into)
{
    if (!from || !into || from == into) return;
    for (const auto &ob : from->_obs) {                                 // key order
        Feature *f = ob.second;
        if (into->_obs.count(ob.first) == 0) {
            if (f) f->_mappoint = into;
            into->_obs[ob.first] = f;
        } else if (f) f->_mappoint = nullptr;
    }
    into->_cnt_found += from->_cnt_found;
    into->_cnt_visible += from->_cnt_visible;
    from->_bad = true;
    from->_obs.clear();
}

// ------------------------------------------------------------------------------------------ LoopClosing::UpdateCovisibility
int LoopClosing::UpdateCovisibility(const vector<Frame *> &rows, const vector<Frame *> &keyframes)
{
    const vector<Frame *> u = universe_of(keyframes);
    const int K = (int)u.size();
    if (K < 1 || rows.empty()) return 0;
    if (K > YGZ_MAP_MAX_KEYFRAMES) {
        LOG(ERROR) << "LoopClosing::UpdateCovisibility: " << K << " keyframes: above the call's capacity" << endl;
        return 0;
    }
    map<unsigned long, int> index;                                      // keyframe id -> universe index (ascending with the id)
    for (int i = 0; i < K; ++i) index[u[i]->_keyframe_id] = i;
    // the rows: those of the universe, once each, by id
    vector<int32_t> row_idx;
    {
        vector<Frame *> r = universe_of(rows);
        for (Frame *k : r) {
            auto it = index.find(k->_keyframe_id);
            if (it != index.end() && u[it->second] == k) row_idx.push_back(it->second);
        }
    }
    if (row_idx.empty()) return 0;
    // the points: keyframes by id, features by index, each good point once; a point's list = its _obs keys of the universe
    vector<int32_t> offsets(1, 0), kf;
    std::set<const MapPoint *> seen;
    for (Frame *k : u)
        for (const Feature *f : k->_features) {
            const MapPoint *mp = f ? f->_mappoint : nullptr;
            if (!good(mp) || !seen.insert(mp).second) continue;
            for (const auto &ob : mp->_obs) {
                auto it = index.find(ob.first);
                if (it != index.end()) kf.push_back(it->second);
            }
            offsets.push_back((int32_t)kf.size());
        }
    const int P = (int)offsets.size() - 1;
    if (P < 1) return 0;
    if (kf.size() > YGZ_MAP_MAX_OBS) {
        LOG(ERROR) << "LoopClosing::UpdateCovisibility: " << kf.size() << " observations: above the call's capacity" << endl;
        return 0;
    }
    if (kf.empty()) return 0;
    const size_t per_call = std::max<size_t>(1, (size_t)YGZ_COVIS_MAX_CELLS / (size_t)K);
    int rewritten = 0;
    vector<int32_t> w;
    for (size_t r0 = 0; r0 < row_idx.size(); r0 += per_call) {
        const size_t nr = std::min(per_call, row_idx.size() - r0);
        w.assign(nr * (size_t)K, 0);
        if (!hip::check(ygz_hip_covisibility(hip::Runtime::Get().ctx(), P, offsets.data(), kf.data(), K, (int)nr, &row_idx[r0], w.data()),
                        "covisibility"))
            return rewritten;
        for (size_t r = 0; r < nr; ++r) {
            Frame *self = u[row_idx[r0 + r]];
            const int32_t *c = &w[r * (size_t)K];
            map<Frame *, int> shared;
            vector<pair<int, Frame *>> wk;                              // universe order = id order
            int best = -1;
            for (int b = 0; b < K; ++b) {
                if (b == row_idx[r0 + r] || c[b] <= 0) continue;
                shared[u[b]] = c[b];
                if (best < 0 || c[b] > c[best]) best = b;               // the first (smallest id) of the largest
                if (c[b] >= kCovisibilityTh) wk.push_back(make_pair((int)c[b], u[b]));
            }
            if (shared.empty()) continue;
            if (wk.empty()) {
                wk.push_back(make_pair((int)c[best], u[best]));
                u[best]->AddConnection(self, c[best]);
            }
            std::stable_sort(wk.begin(), wk.end(), [](const pair<int, Frame *> &a, const pair<int, Frame *> &b) { return a.first > b.first; });
            self->_connected_keyframe_weights = shared;
            self->_cov_keyframes.clear(); self->_cov_weights.clear();
            for (const auto &p : wk) { self->_cov_keyframes.push_back(p.second); self->_cov_weights.push_back(p.first); }
            ++rewritten;
        }
    }
    return rewritten;
}

// ------------------------------------------------------------------------------------------ LoopClosing::FuseLoop
bool LoopClosing::FuseLoop()
{
    vector<Frame *> kfs;
    const int n = Memory::GetNumberFrames();
    for (int id = 0; id < n; ++id) {
        Frame *k = Memory::GetKeyFrame((unsigned long)id);
        if (k) kfs.push_back(k);
    }
    return FuseLoop(kfs);
}

bool LoopClosing::FuseLoop(const vector<Frame *> &keyframes)
{
    if (!_fusable || !_current || !_matched || _current_matched.size() != _current->_features.size()) return false;
    const vector<Frame *> u = universe_of(keyframes);
    if (std::find(u.begin(), u.end(), _current) == u.end()) {
        LOG(ERROR) << "LoopClosing::FuseLoop: the current keyframe is not among the keyframes given" << endl;
        return false;
    }
    _fusable = false;
    _fused.clear();
    _stats.fuse_current_replaced = _stats.fuse_current_added = _stats.fuse_targets = _stats.fuse_hits = _stats.fuse_replaced = 0;
    _stats.fuse_added = _stats.fuse_conflicts = _stats.fuse_descriptors = _stats.fuse_rows = 0;

    std::set<MapPoint *> gained;                                        // loop map points with a new observation
    std::set<Frame *> touched;                                          // keyframes in which a feature's _mappoint changed
    auto frame_of = [](unsigned long id, const Feature *f) -> Frame * { return f && f->_frame ? f->_frame : Memory::GetKeyFrame(id); };
    // q -> L: every keyframe that observes q has a feature that changes; L gains wherever it was not observed
    auto replace = [&](MapPoint *q, MapPoint *L) {
        for (const auto &ob : q->_obs) {
            if (Frame *k = frame_of(ob.first, ob.second)) touched.insert(k);
            if (L->_obs.count(ob.first) == 0) gained.insert(L);
        }
        ReplaceMapPoint(q, L);
    };
    auto add = [&](Frame *k, Feature *f, MapPoint *L) {
        f->_mappoint = L;
        L->_obs[k->_keyframe_id] = f;
        touched.insert(k);
        gained.insert(L);
    };

    // 1. the current keyframe's matches
    Frame *cur = _current;
    for (size_t i = 0; i < _current_matched.size(); ++i) {
        MapPoint *L = _current_matched[i];
        if (!good(L)) continue;
        if (L->_obs.count(cur->_keyframe_id)) { ++_stats.fuse_conflicts; continue; }
        Feature *f = cur->_features[i];
        MapPoint *q = f->_mappoint;
        if (good(q)) {
            const FusedPair fp = { cur->_keyframe_id, (int)i, L->_id, (long)q->_id };
            replace(q, L);
            ++_stats.fuse_current_replaced;
            _fused.push_back(fp);
        } else {
            add(cur, f, L);
            ++_stats.fuse_current_added;
            _fused.push_back(FusedPair{ cur->_keyframe_id, (int)i, L->_id, -1 });
        }
    }

    // 2. the targets: the current keyframe and its connected keyframes (either direction) outside the loop group, by id
    std::set<const Frame *> loop_group;
    loop_group.insert(_matched);
    for (const auto &c : _matched->_connected_keyframe_weights) if (c.first) loop_group.insert(c.first);
    vector<Frame *> targets;
    for (Frame *k : u) {
        if (loop_group.count(k)) continue;
        const bool connected = cur->_connected_keyframe_weights.count(k) > 0 || k->_connected_keyframe_weights.count(cur) > 0;
        if (k == cur || connected) targets.push_back(k);
    }
    _stats.fuse_targets = (int)targets.size();
    vector<vector<int>> hits;
    if (!targets.empty() && !_loop_points.empty()) {
        vector<Sim3> poses;
        for (Frame *k : targets) poses.push_back(Sim3(k->_TCW));
        // SearchFuseCandidates holds YGZ_PROJ_MAX_POINTS points per call: larger sets go in chunks of points
        hits.assign(targets.size(), vector<int>(_loop_points.size(), -1));
        for (size_t p0 = 0; p0 < _loop_points.size(); p0 += YGZ_PROJ_MAX_POINTS) {
            const size_t p1 = std::min(_loop_points.size(), p0 + (size_t)YGZ_PROJ_MAX_POINTS);
            const vector<MapPoint *> part(_loop_points.begin() + p0, _loop_points.begin() + p1);
            vector<vector<int>> h;
            _stats.fuse_hits += _matcher.SearchFuseCandidates(targets, poses, part, _option._fuse_search_th, h);
            for (size_t k = 0; k < h.size() && k < targets.size(); ++k) std::copy(h[k].begin(), h[k].end(), hits[k].begin() + p0);
        }
    }

    // 3. the hits, each against the map as it is now
    std::set<const MapPoint *> is_loop_point(_loop_points.begin(), _loop_points.end());
    for (size_t k = 0; k < hits.size(); ++k) {
        Frame *kf = targets[k];
        for (size_t i = 0; i < hits[k].size(); ++i) {
            const int j = hits[k][i];
            if (j < 0 || j >= (int)kf->_features.size()) continue;
            MapPoint *L = _loop_points[i];
            if (!good(L) || L->_obs.count(kf->_keyframe_id)) { ++_stats.fuse_conflicts; continue; }
            Feature *f = kf->_features[j];
            MapPoint *q = f->_mappoint;
            if (!good(q)) {
                add(kf, f, L);
                ++_stats.fuse_added;
                _fused.push_back(FusedPair{ kf->_keyframe_id, j, L->_id, -1 });
            } else if (q == L) {
                continue;
            } else if (is_loop_point.count(q)) {
                ++_stats.fuse_conflicts;
            } else {
                const FusedPair fp = { kf->_keyframe_id, j, L->_id, (long)q->_id };
                replace(q, L);
                ++_stats.fuse_replaced;
                _fused.push_back(fp);
            }
        }
    }

    // 4. the distinctive descriptor of every loop map point that gained an observation, in the loop map points' order
    vector<MapPoint *> redo;
    for (MapPoint *L : _loop_points) if (gained.count(L)) redo.push_back(L);
    if (!redo.empty()) _stats.fuse_descriptors = _matcher.ComputeDistinctiveDescriptors(redo);

    // 5. the covisibility of every keyframe touched, and of those that observe a point that gained an observation
    for (MapPoint *L : redo)
        for (const auto &ob : L->_obs)
            if (Frame *k = frame_of(ob.first, ob.second)) touched.insert(k);
    vector<Frame *> rows(touched.begin(), touched.end());
    std::sort(rows.begin(), rows.end(), by_id);
    if (!rows.empty()) _stats.fuse_rows = UpdateCovisibility(rows, u);
    return true;
}

}  // namespace ygz
