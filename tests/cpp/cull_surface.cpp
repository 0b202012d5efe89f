// ygz::KeyFrameCulling used the way INTEGRATION.md shows, written against include/ygz only, on a map built by hand (no images): fourteen keyframes
// along a line, the middle ones one unit apart and therefore redundant, the outer ones four units apart; a map point every sixth of a unit seen
// by every keyframe within five units, two private points per neighbouring pair, _obs, _level, _ref_keyframe and the connections filled, a
// hand-filled _bow_vec per keyframe in an attached KeyFrameDatabase.  The same map is also walked by a plain host loop over _obs (expect_walk,
// coded independently of ygz_slam_amd/host/ygz_cull.cpp): Cull has to cull the same keyframes in the same order and kill the same points.
// Built as a shared object by tests/test_cull_surface_build.py (-Wl,--no-undefined) and called through ctypes by tests/cull_driver.py.
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
using namespace ygz;

namespace {

struct World {
    vector<Frame *> kfs;
    vector<MapPoint *> mps;
    vector<Feature *> loose;                            // features without a map point
    ~World()
    {
        for (Frame *k : kfs) delete k;                  // a frame deletes its features
        for (MapPoint *p : mps) delete p;
    }
};

Feature *add_feature(Frame *kf, int level)
{
    Feature *f = new Feature(Vector2d(20.0 + kf->_features.size(), 30.0), level);
    f->_frame = kf;
    kf->_features.push_back(f);
    return f;
}

void observe(MapPoint *p, Frame *kf, int level)
{
    Feature *f = add_feature(kf, level);
    p->_obs[kf->_keyframe_id] = f;
    f->_mappoint = p;
}

// shared points counted over _obs; _connected_keyframe_weights for every pair that shares a point, _cov_keyframes for 15 and more (or the best)
void fill_connections(World &w)
{
    for (Frame *a : w.kfs) {
        map<Frame *, int> shared;
        for (Feature *f : a->_features) {
            if (!f->_mappoint || f->_mappoint->_bad) continue;
            for (const auto &ob : f->_mappoint->_obs)
                if (ob.second->_frame != a) ++shared[ob.second->_frame];
        }
        a->_connected_keyframe_weights = shared;
        vector<pair<int, Frame *>> wk;
        for (Frame *b : w.kfs) if (shared.count(b) && shared[b] >= 15) wk.push_back(make_pair(shared[b], b));
        if (wk.empty())
            for (Frame *b : w.kfs) if (shared.count(b) && (wk.empty() || shared[b] > wk[0].first)) wk.assign(1, make_pair(shared[b], b));
        std::stable_sort(wk.begin(), wk.end(), [](const pair<int, Frame *> &x, const pair<int, Frame *> &y) { return x.first > y.first; });
        a->_cov_keyframes.clear(); a->_cov_weights.clear();
        for (const auto &e : wk) { a->_cov_keyframes.push_back(e.second); a->_cov_weights.push_back(e.first); }
    }
}

// keyframe k at x = pos[k]; _keyframe_id = 100 + 3 k; _id = ids[k]
void build_map(World &w, const vector<int> &pos, const vector<unsigned long> &ids)
{
    const int K = (int)pos.size();
    for (int k = 0; k < K; ++k) {
        Frame *kf = new Frame;
        kf->_keyframe_id = 100 + 3 * (unsigned long)k;
        kf->_id = ids[k];
        kf->_is_keyframe = true;
        const double T[7] = { 0, 0, 0, 1, -(double)pos[k] - 0.125, 0.25 * k, 1.0 / 3.0 };
        kf->_TCW = SE3::from7(T);
        kf->_ref_keyframe = k > 0 ? w.kfs[k - 1] : nullptr;
        kf->_bow_vec[(DBoW3::WordId)k] = 0.5; kf->_bow_vec[(DBoW3::WordId)(k + 1)] = 0.25; kf->_bow_vec[(DBoW3::WordId)(100 + k)] = 0.25;
        w.kfs.push_back(kf);
    }
    unsigned long next_id = 1;
    auto point = [&](double x) {
        MapPoint *p = new MapPoint;
        p->_id = next_id++;
        p->_pos_world = Vector3d(x, 0.1 * (double)(p->_id % 7), 4.0 + 1.0 / (double)p->_id);
        w.mps.push_back(p);
        return p;
    };
    // a point every sixth of a unit, seen within five units
    const int lo = 6 * pos.front() - 30, hi = 6 * pos.back() + 30;
    for (int xi = lo; xi <= hi; ++xi) {
        MapPoint *p = point(xi / 6.0);
        for (int k = 0; k < K; ++k)
            if (std::abs(xi - 6 * pos[k]) <= 30) observe(p, w.kfs[k], (std::abs(xi) + 2 * k) % 5);
    }
    // two private points per neighbouring pair, and two features without a point per keyframe
    for (int k = 0; k + 1 < K; ++k)
        for (int i = 0; i < 2; ++i) {
            MapPoint *p = point(pos[k] + 0.5);
            observe(p, w.kfs[k], i); observe(p, w.kfs[k + 1], i + 1);
        }
    for (Frame *kf : w.kfs) { w.loose.push_back(add_feature(kf, 0)); w.loose.push_back(add_feature(kf, 7)); }
    fill_connections(w);
}

// everything a call may edit, as numbers
vector<long> snapshot(const World &w)
{
    vector<long> s;
    map<const Feature *, long> fid;
    for (const Frame *k : w.kfs)
        for (size_t i = 0; i < k->_features.size(); ++i) fid[k->_features[i]] = (long)k->_keyframe_id * 1000 + (long)i;
    for (const Frame *k : w.kfs) {
        s.push_back(k->_bad); s.push_back((long)k->_id); s.push_back(k->_ref_keyframe ? (long)k->_ref_keyframe->_keyframe_id : -1);
        for (const Frame *b : w.kfs) s.push_back(k->_connected_keyframe_weights.count(const_cast<Frame *>(b)) ? k->_connected_keyframe_weights.at(const_cast<Frame *>(b)) : -1);
        s.push_back((long)k->_connected_keyframe_weights.size());
        s.push_back((long)k->_cov_keyframes.size());
        for (const Frame *b : k->_cov_keyframes) s.push_back((long)b->_keyframe_id);
        for (int v : k->_cov_weights) s.push_back(v);
        for (const Feature *f : k->_features) { s.push_back(f->_mappoint ? (long)f->_mappoint->_id : -1); s.push_back(f->_level); }
    }
    for (const MapPoint *p : w.mps) {
        s.push_back(p->_bad); s.push_back((long)p->_obs.size());
        for (const auto &ob : p->_obs) { s.push_back((long)ob.first); s.push_back(fid.count(ob.second) ? fid[ob.second] : -1); }
    }
    return s;
}

// poses and positions as bytes
vector<double> geometry(const World &w)
{
    vector<double> g;
    for (const Frame *k : w.kfs) { double T[7]; k->_TCW.to7(T); g.insert(g.end(), T, T + 7); }
    for (const MapPoint *p : w.mps) for (int i = 0; i < 3; ++i) g.push_back(p->_pos_world[i]);
    return g;
}
bool same_bytes(const vector<double> &a, const vector<double> &b) { return a.size() == b.size() && memcmp(a.data(), b.data(), 8 * a.size()) == 0; }

struct Expect {
    vector<Frame *> decided, culled;
    vector<int> tracked, redundant;                     // per decided candidate, at its decision
    std::set<MapPoint *> dead;
};

int clamp_level(int l) { return l < 0 ? 0 : l > 15 ? 15 : l; }

// tracked and redundant of c over _obs, with `removed` keyframes and `dead` points left out
void host_counts(Frame *c, const KeyFrameCulling::Options &o, const std::set<Frame *> &removed, const std::set<MapPoint *> &dead, int &tracked,
                 int &redundant)
{
    tracked = redundant = 0;
    for (Feature *f : c->_features) {
        MapPoint *p = f->_mappoint;
        if (!p || p->_bad || dead.count(p)) continue;
        ++tracked;
        int nobs = 0;
        for (const auto &ob : p->_obs) {
            Frame *b = ob.second->_frame;
            if (b == c || b->_bad || removed.count(b)) continue;
            if (o.level_slack >= 0 && clamp_level(ob.second->_level) > clamp_level(f->_level) + o.level_slack) continue;
            ++nobs;
        }
        if (nobs >= o.th_obs) ++redundant;
    }
}

// ORB-SLAM2's walk as a plain loop on the map itself; nothing is edited
Expect expect_walk(const vector<Frame *> &candidates, const vector<Frame *> &keep, const KeyFrameCulling::Options &o)
{
    Expect e;
    std::set<Frame *> removed, visited;
    map<MapPoint *, int> live;
    for (Frame *c : candidates) {
        if (!c || c->_bad || !visited.insert(c).second || c->_id == 0 || std::find(keep.begin(), keep.end(), c) != keep.end()) continue;
        int t = 0, r = 0;
        host_counts(c, o, removed, e.dead, t, r);
        e.decided.push_back(c); e.tracked.push_back(t); e.redundant.push_back(r);
        if (!((double)r > o.ratio * (double)t)) continue;
        e.culled.push_back(c);
        removed.insert(c);
        for (Feature *f : c->_features) {
            MapPoint *p = f->_mappoint;
            if (!p || p->_bad) continue;
            if (!live.count(p)) {
                int n = 0;
                for (const auto &ob : p->_obs) n += !ob.second->_frame->_bad;
                live[p] = n;
            }
            if (--live[p] < o.min_obs) e.dead.insert(p);
        }
    }
    return e;
}

// the invariants of the map after an edit
bool features_and_points_agree(const World &w)
{
    for (const Frame *k : w.kfs)
        for (const Feature *f : k->_features) {
            const MapPoint *p = f->_mappoint;
            if (!p) continue;
            if (p->_bad) return false;
            auto it = p->_obs.find(k->_keyframe_id);
            if (it == p->_obs.end() || it->second != f) return false;
        }
    for (const MapPoint *p : w.mps)
        for (const auto &ob : p->_obs)
            if (!ob.second || ob.second->_mappoint != p || ob.second->_frame->_keyframe_id != ob.first) return false;
    return true;
}

bool no_good_point_names_a_bad_keyframe(const World &w)
{
    for (const MapPoint *p : w.mps)
        for (const auto &ob : p->_obs)
            if (!p->_bad && ob.second->_frame->_bad) return false;
    return true;
}

bool bad_keyframes_are_disconnected(const World &w)
{
    for (const Frame *k : w.kfs) {
        if (k->_bad && !(k->_connected_keyframe_weights.empty() && k->_cov_keyframes.empty() && k->_cov_weights.empty())) return false;
        if (k->_cov_keyframes.size() != k->_cov_weights.size()) return false;
        for (const auto &c : k->_connected_keyframe_weights) if (c.first->_bad) return false;
        for (const Frame *c : k->_cov_keyframes) if (c->_bad) return false;
    }
    return true;
}

bool dead_points_equal(const World &w, const std::set<MapPoint *> &bad_before, const std::set<MapPoint *> &dead)
{
    for (MapPoint *p : w.mps)
        if ((p->_bad && !bad_before.count(p)) != (dead.count(p) > 0)) return false;
    return true;
}

std::set<MapPoint *> bad_points(const World &w)
{
    std::set<MapPoint *> s;
    for (MapPoint *p : w.mps) if (p->_bad) s.insert(p);
    return s;
}

// Cull against the host loop on the map as it is: the same keyframes in the same order, the same points killed, the statistics
bool cull_equals_host(World &w, KeyFrameCulling &kc, const vector<Frame *> &candidates, const vector<Frame *> &keep, int *n_culled, int *n_killed)
{
    const Expect e = expect_walk(candidates, keep, kc._options);
    const std::set<MapPoint *> before = bad_points(w);
    vector<Frame *> culled;
    const int n = kc.Cull(candidates, &culled);
    const KeyFrameCulling::Stats &st = kc.GetStats();
    if (n_culled) *n_culled = n;
    if (n_killed) *n_killed = st.points_killed;
    bool ok = n == (int)e.culled.size() && culled == e.culled && dead_points_equal(w, before, e.dead);
    ok = ok && st.culled == n && st.candidates == (int)e.decided.size() && st.skipped == (int)candidates.size() - st.candidates;
    ok = ok && st.points_killed == (int)e.dead.size() && st.dead_mismatch == 0;
    for (Frame *k : e.culled) ok = ok && k->_bad;
    return ok;
}

const vector<int> kLine = { 0, 4, 8, 9, 10, 11, 12, 13, 14, 15, 16, 20, 24, 28 };
// keyframe 6 (x = 12, the middle of the dense stretch) is the map's first frame
const vector<unsigned long> kIds = { 8, 9, 10, 11, 12, 13, 0, 1, 2, 3, 4, 5, 6, 7 };

}  // namespace

extern "C" {

// checks [32] (all of the first N_CHECKS must be 1), info [16]:
//   0 Redundancy equals the host loop's counts for every keyframe, zeros for a null entry      1 Redundancy changed nothing
//   2 the keyframe with _id == 0 and the protected one are redundant on the initial map        3 Cull culled something and kept something
//   4 Cull equals the host loop: keyframes, order, killed points, statistics                   5 points were killed
//   6 f->_mappoint == p exactly when p->_obs[id(f)] == f, no feature points to a bad point     7 no good point's _obs names a bad keyframe
//   8 no culled keyframe is in any _cov_keyframes / _connected_keyframe_weights, its own are empty
//   9 the database's Size() fell by the number culled, culled keyframes are not held          10 Stats: universe, points, observations, db_erased
//  11 UpdateCovisibility(all, all) reproduces the edited _connected_keyframe_weights of every survivor
//  12 the keyframe with _id == 0 and the protected one survive                                13 poses and point positions are bit-unchanged
//  14 _ref_keyframe of every survivor is its nearest surviving ancestor                        15 a second Cull over the survivors equals the host loop again
//  16 a universe of five keyframes: 0, the map unchanged                                      17 level_slack = 1: Cull equals the host loop
//  18 three candidates only: the observers outside the list are in the universe, Cull equals the host loop
//  19 min_obs = 0: nothing is killed, Cull equals the host loop
//   info: 0 culled (main), 1 points killed (main), 2 universe, 3 points, 4 observations, 5 culled in the second round, 6 culled with slack 1,
//   7 culled of three candidates, 8 universe of that call
// Returns 0, 1 on an exception.
int cull_run(double *checks, double *info)
{
    for (int i = 0; i < 32; ++i) checks[i] = 0;
    for (int i = 0; i < 16; ++i) info[i] = 0;
    try {
        Config::Set("image.width", "640"); Config::Set("image.height", "480");
        {   // the main map
            World w;
            build_map(w, kLine, kIds);
            KeyFrameDatabase db;
            bool added = true;
            for (Frame *k : w.kfs) added = added && db.Add(k);
            KeyFrameCulling kc;
            kc.SetKeyFrameDatabase(&db);
            Frame *first = w.kfs[6], *kept = w.kfs[5];
            kc.SetProtected({ kept });
            const vector<double> geo = geometry(w);
            const vector<long> snap = snapshot(w);

            vector<Frame *> ask = w.kfs;
            ask.insert(ask.begin() + 2, nullptr);
            vector<KeyFrameCulling::Entry> red;
            bool ok = kc.Redundancy(ask, red) && red.size() == ask.size();
            const std::set<Frame *> none;
            const std::set<MapPoint *> no_points;
            bool any_redundant = false;
            for (size_t i = 0; ok && i < ask.size(); ++i) {
                int t = 0, r = 0;
                if (ask[i]) host_counts(ask[i], kc._options, none, no_points, t, r);
                ok = red[i].kf == ask[i] && red[i].tracked == t && red[i].redundant == r && (ask[i] == nullptr || t > 0);
                any_redundant = any_redundant || r > 0;
            }
            checks[0] = ok && any_redundant;
            checks[1] = snapshot(w) == snap && same_bytes(geometry(w), geo);
            {
                int t0 = 0, r0 = 0, t1 = 0, r1 = 0;
                host_counts(first, kc._options, none, no_points, t0, r0);
                host_counts(kept, kc._options, none, no_points, t1, r1);
                checks[2] = first->_id == 0 && (double)r0 > kc._options.ratio * (double)t0 && (double)r1 > kc._options.ratio * (double)t1;
            }

            // the decision order: the dense stretch first, a null and a repeat among them
            vector<Frame *> order = { w.kfs[6], w.kfs[5], w.kfs[7], nullptr, w.kfs[8], w.kfs[4], w.kfs[7], w.kfs[3], w.kfs[9], w.kfs[0], w.kfs[1],
                                      w.kfs[2], w.kfs[10], w.kfs[11], w.kfs[12], w.kfs[13] };
            const size_t db_before = db.Size();
            int n = 0, killed = 0;
            checks[4] = cull_equals_host(w, kc, order, { kept }, &n, &killed);
            const KeyFrameCulling::Stats st = kc.GetStats();
            info[0] = n; info[1] = killed; info[2] = st.universe; info[3] = st.points; info[4] = st.observations;
            checks[3] = n > 0 && n < (int)w.kfs.size() - 2;
            checks[5] = killed > 0;
            checks[6] = features_and_points_agree(w);
            checks[7] = no_good_point_names_a_bad_keyframe(w);
            checks[8] = bad_keyframes_are_disconnected(w);
            bool held = added && db.Size() + (size_t)n == db_before && st.db_erased == n;
            for (Frame *k : w.kfs) held = held && db.Has(k) == !k->_bad;
            checks[9] = held;
            size_t n_obs = 0;
            for (MapPoint *p : w.mps) n_obs += p->_obs.size();
            checks[10] = st.universe == (int)w.kfs.size() && st.points == (int)w.mps.size() && st.observations > st.points && n_obs < (size_t)st.observations;
            {   // the weights the edit left are the weights a recount gives
                vector<map<Frame *, int>> edited;
                for (Frame *k : w.kfs) edited.push_back(k->_connected_keyframe_weights);
                LoopClosing lc;
                const int rows = lc.UpdateCovisibility(w.kfs, w.kfs);
                bool same = rows > 0;
                for (size_t k = 0; k < w.kfs.size(); ++k) same = same && (w.kfs[k]->_bad || w.kfs[k]->_connected_keyframe_weights == edited[k]);
                checks[11] = same && bad_keyframes_are_disconnected(w);
            }
            checks[12] = !first->_bad && !kept->_bad;
            checks[13] = same_bytes(geometry(w), geo);
            {
                bool refs = true;
                Frame *last_alive = nullptr;
                for (Frame *k : w.kfs) {                                // the chain of build_map: k refers to k - 1
                    if (!k->_bad) { refs = refs && k->_ref_keyframe == last_alive; last_alive = k; }
                }
                checks[14] = refs;
            }
            vector<Frame *> again;
            for (Frame *k : w.kfs) again.push_back(k);                   // bad ones among them: skipped
            int n2 = 0;
            checks[15] = cull_equals_host(w, kc, again, { kept }, &n2, nullptr) && features_and_points_agree(w) && no_good_point_names_a_bad_keyframe(w)
                         && bad_keyframes_are_disconnected(w) && same_bytes(geometry(w), geo);
            info[5] = n2;
        }
        {   // five keyframes, three of them at one place and redundant: none culled
            World w;
            build_map(w, { 0, 1, 1, 1, 2 }, { 1, 2, 3, 4, 5 });
            KeyFrameCulling kc;
            const vector<long> snap = snapshot(w);
            const Expect e = expect_walk(w.kfs, {}, kc._options);
            vector<Frame *> culled(1, w.kfs[0]);
            const int n = kc.Cull(w.kfs, &culled);
            checks[16] = n == 0 && culled.empty() && !e.culled.empty() && kc.GetStats().universe == 5 && snapshot(w) == snap;
        }
        {   // ORB-SLAM2's scale test
            World w;
            build_map(w, kLine, kIds);
            KeyFrameCulling::Options o;
            o.level_slack = 1; o.ratio = 0.5;
            KeyFrameCulling kc(o);
            int n = 0;
            vector<Frame *> order(w.kfs.rbegin(), w.kfs.rend());
            checks[17] = cull_equals_host(w, kc, order, {}, &n, nullptr) && n > 0 && features_and_points_agree(w) && bad_keyframes_are_disconnected(w);
            info[6] = n;
        }
        {   // three candidates: their points' other observers count and keep points alive
            World w;
            build_map(w, kLine, kIds);
            KeyFrameCulling kc;
            int n = 0;
            checks[18] = cull_equals_host(w, kc, { w.kfs[8], w.kfs[4], w.kfs[7] }, {}, &n, nullptr) && n > 0 && kc.GetStats().universe > 3
                         && features_and_points_agree(w) && no_good_point_names_a_bad_keyframe(w) && bad_keyframes_are_disconnected(w);
            info[7] = n; info[8] = kc.GetStats().universe;
        }
        {   // min_obs = 0: points outlive their observers
            World w;
            build_map(w, kLine, kIds);
            KeyFrameCulling::Options o;
            o.min_obs = 0;
            KeyFrameCulling kc(o);
            int n = 0, killed = -1;
            checks[19] = cull_equals_host(w, kc, w.kfs, {}, &n, &killed) && n > 0 && killed == 0 && bad_points(w).empty() && features_and_points_agree(w);
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "cull_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // extern "C"
