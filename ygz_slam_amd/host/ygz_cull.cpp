// ygz::KeyFrameCulling (include/ygz/Algorithm/KeyFrameCulling.h): the reference has the stage written and switched off (LocalMapping.cpp:579-618);
// ORB-SLAM2's LocalMapping::KeyFrameCulling and KeyFrame::SetBadFlag on this data model.  The observation lists of the candidates' map points go
// to the device once; the counts (ygz_hip_keyframe_redundancy) and the whole sequential walk (ygz_hip_cull_keyframes, ygz_slam_amd/csrc/cull.hip)
// are one call each, and the map is edited on the host afterwards.  Every order goes by keyframe id or index.  Error conventions of the other
// surfaces: a failed call logs and returns 0 / false, only a missing device throws.
#include "ygz/Algorithm/KeyFrameCulling.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include <algorithm>

namespace ygz {

namespace {
bool by_id(const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; }
using hip::good;

void disconnect(Frame *k, const Frame *gone)
{
    k->_connected_keyframe_weights.erase(const_cast<Frame *>(gone));
    for (size_t i = 0; i < k->_cov_keyframes.size();) {
        if (k->_cov_keyframes[i] != gone) { ++i; continue; }
        k->_cov_keyframes.erase(k->_cov_keyframes.begin() + i);
        if (i < k->_cov_weights.size()) k->_cov_weights.erase(k->_cov_weights.begin() + i);
    }
}
}

// the device call's input: the universe, the points and their lists
struct KeyFrameCulling::Problem {
    vector<Frame *> valid;                  // given, non-null, not bad, once each (the first wins), in the order given
    vector<Frame *> universe;               // by _keyframe_id
    map<const Frame *, int> index;          // lookups only: nothing is ordered by it
    vector<MapPoint *> points;
    vector<int32_t> offsets, kf, level;
};

void KeyFrameCulling::SetProtected(const vector<Frame *> &keyframes)
{
    _protected.clear();
    for (Frame *k : keyframes) if (k) _protected.push_back(k);
}

bool KeyFrameCulling::Build(const vector<Frame *> &given, Problem &pb, const char *who)
{
    std::set<const Frame *> in;
    for (Frame *k : given) if (k && !k->_bad && in.insert(k).second) pb.valid.push_back(k);
    vector<Frame *> by = pb.valid;
    std::stable_sort(by.begin(), by.end(), by_id);
    // the universe: the given keyframes and every other observer of their good map points
    pb.universe = by;
    for (Frame *k : by)
        for (const Feature *f : k->_features) {
            const MapPoint *mp = f ? f->_mappoint : nullptr;
            if (!good(mp)) continue;
            for (const auto &ob : mp->_obs) {
                Frame *o = ob.second ? ob.second->_frame : nullptr;
                if (o && !o->_bad && in.insert(o).second) pb.universe.push_back(o);
            }
        }
    std::stable_sort(pb.universe.begin(), pb.universe.end(), by_id);
    if (pb.universe.size() > (size_t)YGZ_CULL_MAX_KEYFRAMES) {
        LOG(ERROR) << "KeyFrameCulling::" << who << ": " << pb.universe.size() << " keyframes: above the call's capacity" << endl;
        return false;
    }
    for (size_t i = 0; i < pb.universe.size(); ++i) pb.index[pb.universe[i]] = (int)i;
    // the points: given keyframes by id, features by index, each good point once
    pb.offsets.assign(1, 0);
    std::set<const MapPoint *> seen;
    vector<pair<int, int>> list;
    for (Frame *k : by)
        for (const Feature *f : k->_features) {
            MapPoint *mp = f ? f->_mappoint : nullptr;
            if (!good(mp) || !seen.insert(mp).second) continue;
            list.clear();
            for (const auto &ob : mp->_obs) {                           // key order
                const Feature *g = ob.second;
                if (!g || !g->_frame) continue;
                auto it = pb.index.find(g->_frame);
                if (it != pb.index.end()) list.push_back(make_pair(it->second, std::min(15, std::max(0, g->_level))));
            }
            // universe indices ascend with the keyframe id, as the keys do; a map whose keys and frames disagree is put in order here
            std::sort(list.begin(), list.end());
            bool twice = false;
            for (size_t i = 1; i < list.size(); ++i) twice = twice || list[i].first == list[i - 1].first;
            if (twice || list.size() > (size_t)YGZ_MAP_MAX_OBS_PER_POINT) {
                LOG(ERROR) << "KeyFrameCulling::" << who << ": map point " << mp->_id << " has " << list.size() << " observations"
                           << (twice ? ", two of one keyframe" : ": above the call's capacity") << endl;
                return false;
            }
            for (const auto &e : list) { pb.kf.push_back(e.first); pb.level.push_back(e.second); }
            pb.points.push_back(mp);
            pb.offsets.push_back((int32_t)pb.kf.size());
        }
    if (pb.kf.size() > (size_t)YGZ_MAP_MAX_OBS) {
        LOG(ERROR) << "KeyFrameCulling::" << who << ": " << pb.kf.size() << " observations: above the call's capacity" << endl;
        return false;
    }
    return true;
}

// ------------------------------------------------------------------------------------------ KeyFrameCulling::Redundancy
bool KeyFrameCulling::Redundancy(const vector<Frame *> &kfs, vector<Entry> &out)
{
    out.clear();
    Problem pb;
    if (!Build(kfs, pb, "Redundancy")) return false;
    const int K = (int)pb.universe.size(), P = (int)pb.points.size();
    vector<int32_t> tracked((size_t)std::max(K, 1), 0), redundant((size_t)std::max(K, 1), 0);
    if (K > 0 && P > 0 && !pb.kf.empty()) {
        ygz_cull_params q;
        ygz_hip_default_cull_params(&q);
        q.th_obs = _options.th_obs; q.ratio = _options.ratio; q.level_slack = _options.level_slack; q.min_obs = _options.min_obs;
        if (!hip::check(ygz_hip_keyframe_redundancy(hip::Runtime::Get().ctx(), P, pb.offsets.data(), pb.kf.data(), pb.level.data(), K, &q,
                                                    tracked.data(), redundant.data()), "keyframe_redundancy"))
            return false;
    }
    for (Frame *k : kfs) {
        Entry e = { k, 0, 0 };
        auto it = k && !k->_bad ? pb.index.find(k) : pb.index.end();
        if (it != pb.index.end()) { e.tracked = tracked[it->second]; e.redundant = redundant[it->second]; }
        out.push_back(e);
    }
    return true;
}

// ------------------------------------------------------------------------------------------ KeyFrameCulling::SetBadFlag
void KeyFrameCulling::SetBadFlag(Frame *kf, int min_obs)
{
    if (!kf || kf->_bad) return;
    // either direction: the keyframes kf names, and the keyframes that may name kf because they share a map point with it
    vector<Frame *> peers;
    for (const auto &c : kf->_connected_keyframe_weights) if (c.first && c.first != kf) peers.push_back(c.first);
    for (Frame *c : kf->_cov_keyframes) if (c && c != kf) peers.push_back(c);
    for (Feature *f : kf->_features) {                                  // index order
        MapPoint *p = f ? f->_mappoint : nullptr;
        if (!p) continue;
        for (const auto &ob : p->_obs)
            if (ob.second && ob.second->_frame && ob.second->_frame != kf) peers.push_back(ob.second->_frame);
        auto it = p->_obs.find(kf->_keyframe_id);
        if (it != p->_obs.end() && it->second == f) p->_obs.erase(it);
        f->_mappoint = nullptr;
        if (p->_bad || (long)p->_obs.size() >= (long)min_obs) continue;
        p->_bad = true;
        for (const auto &ob : p->_obs)
            if (ob.second && ob.second->_mappoint == p) ob.second->_mappoint = nullptr;
        p->_obs.clear();
    }
    kf->_bad = true;
    for (Frame *c : peers) disconnect(c, kf);
    kf->_connected_keyframe_weights.clear();
    kf->_cov_keyframes.clear();
    kf->_cov_weights.clear();
}

// ------------------------------------------------------------------------------------------ KeyFrameCulling::Cull
int KeyFrameCulling::Cull(const vector<Frame *> &candidates, vector<Frame *> *culled)
{
    _stats = Stats();
    if (culled) culled->clear();
    Problem pb;
    if (!Build(candidates, pb, "Cull")) return 0;
    const int K = (int)pb.universe.size(), P = (int)pb.points.size();
    _stats.universe = K; _stats.points = P; _stats.observations = (int)pb.kf.size();
    // the walk's candidates, in the caller's order
    vector<Frame *> decide;
    vector<int32_t> cand;
    for (Frame *k : pb.valid) {
        if (k->_id == 0 || std::find(_protected.begin(), _protected.end(), k) != _protected.end()) continue;
        decide.push_back(k);
        cand.push_back(pb.index[k]);
    }
    _stats.candidates = (int)decide.size();
    _stats.skipped = (int)candidates.size() - _stats.candidates;
    if ((size_t)K <= _options.min_keyframes || decide.empty() || P < 1 || pb.kf.empty()) return 0;

    ygz_cull_params q;
    ygz_hip_default_cull_params(&q);
    q.th_obs = _options.th_obs; q.ratio = _options.ratio; q.level_slack = _options.level_slack; q.min_obs = _options.min_obs;
    const size_t C = cand.size();
    vector<int32_t> hit(C, 0), tracked(C, 0), redundant(C, 0);
    vector<uint8_t> dead((size_t)P, 0);
    if (!hip::check(ygz_hip_cull_keyframes(hip::Runtime::Get().ctx(), P, pb.offsets.data(), pb.kf.data(), pb.level.data(), K, (int)C, cand.data(), &q,
                                           hit.data(), tracked.data(), redundant.data(), dead.data()), "cull_keyframes"))
        return 0;

    std::set<const Frame *> gone;
    vector<Frame *> removed;
    for (size_t i = 0; i < C; ++i) if (hit[i]) { removed.push_back(decide[i]); gone.insert(decide[i]); }
    for (Frame *k : removed) {
        SetBadFlag(k, _options.min_obs);
        for (Frame *o : pb.universe) if (o != k) disconnect(o, k);       // one-sided connections SetBadFlag cannot see from k
    }
    for (int p = 0; p < P; ++p) {
        const bool host_dead = pb.points[p]->_bad;
        _stats.points_killed += host_dead;
        _stats.dead_mismatch += host_dead != (dead[p] != 0);
    }
    // the spanning tree: a keyframe that referred to a culled one refers to its first ancestor that is not bad
    for (Frame *o : pb.universe) {
        if (o->_bad || !o->_ref_keyframe || !gone.count(o->_ref_keyframe)) continue;
        Frame *r = o->_ref_keyframe;
        for (int steps = 0; r && r->_bad; ++steps) r = steps < K ? r->_ref_keyframe : nullptr;
        o->_ref_keyframe = r == o ? nullptr : r;
    }
    for (Frame *k : removed)
        if (_db && _db->Has(k) && _db->Erase(k)) ++_stats.db_erased;
    _stats.culled = (int)removed.size();
    if (culled) *culled = removed;
    return _stats.culled;
}

}  // namespace ygz
