// LoopClosing::ReplaceMapPoint on a handful of frames, features and map points built by hand: pure host code, no device is initialised
// (nothing here reaches Runtime::ctx()).  Written against include/ygz only.  Each check prints "<name> ok" or "<name> FAILED"; the program exits
// with the number of failed checks.  Built and run by tests/test_fuse_host.py.
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
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
    MapPoint *point(unsigned long id, int found, int visible)
    {
        MapPoint *p = new MapPoint;
        p->_id = id; p->_cnt_found = found; p->_cnt_visible = visible;
        points.push_back(p);
        return p;
    }
    void observe(MapPoint *p, Feature *f) { p->_obs[f->_frame->_keyframe_id] = f; f->_mappoint = p; }
    // f->_mappoint == p exactly when p->_obs[id(f)] == f, and no feature points to a bad point
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
                if (!ob.second || ob.second->_mappoint != p || ob.second->_frame->_keyframe_id != ob.first) return false;
        return true;
    }
};
}

int main()
{
    {   // disjoint keyframes: every observation moves over
        World w;
        Feature *a0 = w.feature(0), *a1 = w.feature(1), *b2 = w.feature(2), *b3 = w.feature(3);
        MapPoint *into = w.point(1, 3, 5), *from = w.point(2, 4, 7);
        w.observe(into, a0); w.observe(into, a1); w.observe(from, b2); w.observe(from, b3);
        LoopClosing::ReplaceMapPoint(from, into);
        check("disjoint_moved", into->_obs.size() == 4 && into->_obs[12] == b2 && into->_obs[13] == b3 && b2->_mappoint == into && b3->_mappoint == into);
        check("disjoint_kept", into->_obs[10] == a0 && into->_obs[11] == a1 && a0->_mappoint == into && a1->_mappoint == into);
        check("counters_summed", into->_cnt_found == 7 && into->_cnt_visible == 12);
        check("from_bad_and_empty", from->_bad && from->_obs.empty() && !into->_bad);
        check("disjoint_invariant", w.invariant());
    }
    {   // a shared keyframe: `into` keeps its own feature there, from's feature loses its point
        World w;
        Feature *a0 = w.feature(0), *a1 = w.feature(1), *b1 = w.feature(1), *b2 = w.feature(2);
        MapPoint *into = w.point(1, 1, 1), *from = w.point(2, 2, 2);
        w.observe(into, a0); w.observe(into, a1); w.observe(from, b1); w.observe(from, b2);
        LoopClosing::ReplaceMapPoint(from, into);
        check("shared_keeps_own", into->_obs.size() == 3 && into->_obs[11] == a1 && a1->_mappoint == into);
        check("shared_feature_loses_point", b1->_mappoint == nullptr);
        check("shared_other_moves", into->_obs[12] == b2 && b2->_mappoint == into && into->_obs[10] == a0);
        check("shared_from_bad_and_empty", from->_bad && from->_obs.empty());
        check("shared_counters_summed", into->_cnt_found == 3 && into->_cnt_visible == 3);
        check("shared_invariant", w.invariant());
    }
    {   // from == into, and null arguments: nothing happens
        World w;
        Feature *a0 = w.feature(0), *a1 = w.feature(1);
        MapPoint *p = w.point(1, 2, 3), *q = w.point(2, 1, 1);
        w.observe(p, a0); w.observe(q, a1);
        LoopClosing::ReplaceMapPoint(p, p);
        check("same_point_untouched", !p->_bad && p->_obs.size() == 1 && p->_obs[10] == a0 && a0->_mappoint == p && p->_cnt_found == 2 && p->_cnt_visible == 3);
        LoopClosing::ReplaceMapPoint(nullptr, p);
        LoopClosing::ReplaceMapPoint(q, nullptr);
        check("null_untouched", !p->_bad && !q->_bad && p->_obs.size() == 1 && q->_obs.size() == 1 && a1->_mappoint == q && p->_cnt_found == 2);
        check("same_invariant", w.invariant());
    }
    {   // a chain: c into b, then b into a; nothing is deleted, every feature ends on a
        World w;
        Feature *f0 = w.feature(0), *f1 = w.feature(1), *f2 = w.feature(2);
        MapPoint *a = w.point(1, 1, 1), *b = w.point(2, 1, 1), *c = w.point(3, 1, 1);
        w.observe(a, f0); w.observe(b, f1); w.observe(c, f2);
        LoopClosing::ReplaceMapPoint(c, b);
        LoopClosing::ReplaceMapPoint(b, a);
        check("chain", a->_obs.size() == 3 && f0->_mappoint == a && f1->_mappoint == a && f2->_mappoint == a && b->_bad && c->_bad && a->_cnt_found == 3);
        check("chain_invariant", w.invariant());
    }
    return g_failed;
}
