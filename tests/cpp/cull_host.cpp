// KeyFrameCulling::SetBadFlag on a handful of frames, features and map points built by hand: pure host code, no device is initialised
// (nothing here reaches Runtime::ctx()).  Written against include/ygz only.  Each check prints "<name> ok" or "<name> FAILED"; the program exits
// with the number of failed checks.  Built and run by tests/test_cull_host.py.
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <algorithm>
#include <cstdio>
using namespace ygz;

namespace {
int g_failed = 0;
void check(const char *name, bool ok)
{
    printf("%s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) ++g_failed;
}

struct World {
    Frame kf[4];
    vector<Feature *> features;
    vector<MapPoint *> points;
    World() { for (int k = 0; k < 4; ++k) { kf[k]._keyframe_id = kf[k]._id = 10 + k; kf[k]._is_keyframe = true; } }
    ~World() { for (Feature *f : features) delete f; for (MapPoint *p : points) delete p; for (Frame &k : kf) k._features.clear(); }
    Feature *feature(int k)
    {
        Feature *f = new Feature(Vector2d(10.0 * features.size(), 5.0), 0);
        f->_frame = &kf[k];
        kf[k]._features.push_back(f);
        features.push_back(f);
        return f;
    }
    MapPoint *point(unsigned long id)
    {
        MapPoint *p = new MapPoint;
        p->_id = id;
        points.push_back(p);
        return p;
    }
    void observe(MapPoint *p, Feature *f) { p->_obs[f->_frame->_keyframe_id] = f; f->_mappoint = p; }
    void connect(int a, int b, int w, bool both = true)
    {
        kf[a]._connected_keyframe_weights[&kf[b]] = w; kf[a]._cov_keyframes.push_back(&kf[b]); kf[a]._cov_weights.push_back(w);
        if (both) connect(b, a, w, false);
    }
    bool names(int a, int b) const
    {
        const Frame &k = kf[a];
        return k._connected_keyframe_weights.count(const_cast<Frame *>(&kf[b])) > 0
               || std::find(k._cov_keyframes.begin(), k._cov_keyframes.end(), &kf[b]) != k._cov_keyframes.end();
    }
    // f->_mappoint == p exactly when p->_obs[id(f)] == f, no feature points to a bad point, no good point names a bad keyframe
    bool invariant() const
    {
        for (const Feature *f : features) {
            const MapPoint *p = f->_mappoint;
            if (!p) continue;
            if (p->_bad) return false;
            auto it = p->_obs.find(f->_frame->_keyframe_id);
            if (it == p->_obs.end() || it->second != f) return false;
        }
        for (const MapPoint *p : points)
            for (const auto &ob : p->_obs)
                if (!ob.second || ob.second->_mappoint != p || ob.second->_frame->_keyframe_id != ob.first || (!p->_bad && ob.second->_frame->_bad))
                    return false;
        return true;
    }
};
}

int main()
{
    {   // keyframe 1 goes: p (three observers) stays with two, q (two observers) drops under min_obs = 2 and releases keyframe 2's feature
        World w;
        Feature *p0 = w.feature(0), *p1 = w.feature(1), *p2 = w.feature(2), *q1 = w.feature(1), *q2 = w.feature(2), *free1 = w.feature(1);
        MapPoint *p = w.point(1), *q = w.point(2);
        w.observe(p, p0); w.observe(p, p1); w.observe(p, p2); w.observe(q, q1); w.observe(q, q2);
        w.connect(0, 1, 1); w.connect(1, 2, 2); w.connect(0, 2, 1);
        w.connect(3, 1, 7, false);                                      // one-sided: keyframe 3 names keyframe 1 only
        KeyFrameCulling::SetBadFlag(&w.kf[1], 2);
        check("observation_erased", p->_obs.size() == 2 && p->_obs.count(11) == 0 && p->_obs[10] == p0 && p->_obs[12] == p2 && p1->_mappoint == nullptr);
        check("survivor_point_stays", !p->_bad && p0->_mappoint == p && p2->_mappoint == p);
        check("point_under_min_obs_goes_bad", q->_bad && q->_obs.empty() && q1->_mappoint == nullptr);
        check("other_feature_released", q2->_mappoint == nullptr);
        check("feature_without_point_untouched", free1->_mappoint == nullptr && w.kf[1]._features.size() == 3);
        check("keyframe_bad", w.kf[1]._bad && !w.kf[0]._bad && !w.kf[2]._bad && !w.kf[3]._bad);
        check("own_connections_cleared", w.kf[1]._connected_keyframe_weights.empty() && w.kf[1]._cov_keyframes.empty() && w.kf[1]._cov_weights.empty());
        check("connections_removed_on_both_sides", !w.names(0, 1) && !w.names(2, 1) && w.kf[0]._cov_keyframes.size() == 1 && w.kf[0]._cov_weights.size() == 1
                                                   && w.kf[2]._cov_keyframes.size() == 1 && w.kf[2]._cov_weights.size() == 1);
        check("survivors_stay_connected", w.names(0, 2) && w.names(2, 0) && w.kf[0]._connected_keyframe_weights[&w.kf[2]] == 1 && w.kf[2]._cov_weights[0] == 1);
        check("one_sided_connection_named_by_the_keyframe", w.names(3, 1));   // keyframe 3 shares no point with 1 and 1 does not name it: out of SetBadFlag's reach
        check("invariant", w.invariant());
        // a second call is a no-op
        const size_t n_p = p->_obs.size();
        KeyFrameCulling::SetBadFlag(&w.kf[1], 2);
        check("second_call_is_a_no_op", w.kf[1]._bad && p->_obs.size() == n_p && !p->_bad && p0->_mappoint == p && w.names(0, 2) && w.invariant());
    }
    {   // a keyframe that names the culled one without being named, but shares a point with it, is reached through the point
        World w;
        Feature *a0 = w.feature(0), *a1 = w.feature(1), *a2 = w.feature(2);
        MapPoint *p = w.point(1);
        w.observe(p, a0); w.observe(p, a1); w.observe(p, a2);
        w.connect(0, 1, 1, false);
        KeyFrameCulling::SetBadFlag(&w.kf[1], 2);
        check("one_sided_through_a_shared_point", !w.names(0, 1) && w.kf[0]._cov_keyframes.empty() && w.kf[0]._cov_weights.empty());
    }
    {   // min_obs = 0: no point dies; min_obs = 3: a point left with two observers dies
        World w;
        Feature *a0 = w.feature(0), *a1 = w.feature(1), *b1 = w.feature(1), *b2 = w.feature(2), *b3 = w.feature(3);
        MapPoint *a = w.point(1), *b = w.point(2);
        w.observe(a, a0); w.observe(a, a1); w.observe(b, b1); w.observe(b, b2); w.observe(b, b3);
        KeyFrameCulling::SetBadFlag(&w.kf[1], 0);
        check("min_obs_0_keeps_points", !a->_bad && !b->_bad && a->_obs.size() == 1 && a0->_mappoint == a && b->_obs.size() == 2 && w.invariant());
        KeyFrameCulling::SetBadFlag(&w.kf[3], 3);
        check("min_obs_3_kills_a_point_of_one", b->_bad && b->_obs.empty() && b2->_mappoint == nullptr && b3->_mappoint == nullptr && !a->_bad && w.invariant());
    }
    {   // an _obs entry of the keyframe's id that is another feature is not erased; a bad point is only let go; null does nothing
        World w;
        Feature *x1 = w.feature(1), *y1 = w.feature(1), *z1 = w.feature(1), *x0 = w.feature(0), *x2 = w.feature(2);
        MapPoint *p = w.point(1), *dead = w.point(2);
        w.observe(p, x0); w.observe(p, x1); w.observe(p, x2);
        y1->_mappoint = p;                                              // a stale pointer: p's entry for keyframe 11 is x1
        dead->_bad = true; z1->_mappoint = dead;
        KeyFrameCulling::SetBadFlag(nullptr, 2);
        KeyFrameCulling::SetBadFlag(&w.kf[1], 2);
        check("stale_and_bad_points_let_go", x1->_mappoint == nullptr && y1->_mappoint == nullptr && z1->_mappoint == nullptr && p->_obs.size() == 2 && !p->_bad
                                             && dead->_bad && w.invariant());
    }
    return g_failed;
}
