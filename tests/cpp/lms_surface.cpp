// ygz::LocalMapSelector against StereoTracker::LocalKeyFrames, written against include/ygz only.  The same small map is built twice by hand:
// six keyframes (ids 20 .. 25, keyframe 24 bad) with their covisible lists (one of them holds a null), sixteen map points (one bad) and four
// tracked frames -- frames 0 and 1 see points of the same keyframes, frame 2 carries a point twice and the bad point, frame 3 has features and
// no map point.  On one copy StereoTracker::LocalKeyFrames runs frame by frame and the point set of DESIGN.md section 28 is formed with a
// std::set, first occurrence first; on the other ONE LocalMapSelector::Select runs.  Each check prints "<name> ok" or "<name> FAILED"; the
// program exits with the number of failed checks.  `lms_surface run` needs the device; without an argument it prints its usage.  Built by
// tests/test_lms_surface_build.py, run by tests/test_gpu_lms_surface.py.
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <cstdio>
#include <cstring>
#include <set>
#include <sstream>
using namespace ygz;

namespace {
int g_failed = 0;
void check(const char *name, bool ok)
{
    printf("%s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) ++g_failed;
}

const int NK = 6, NF = 4, NP = 16;

struct World {
    Frame kf[NK], fr[NF];
    vector<Feature *> features;
    vector<MapPoint *> points;
    World()
    {
        for (int k = 0; k < NK; ++k) { kf[k]._keyframe_id = kf[k]._id = 20 + k; kf[k]._is_keyframe = true; }
        for (int f = 0; f < NF; ++f) fr[f]._id = 100 + f;
        for (int p = 0; p < NP; ++p) { MapPoint *mp = new MapPoint; mp->_id = 500 + p; points.push_back(mp); }
        // which keyframes see which point, in feature order per keyframe: a gap feature without a point after every third
        const int sees[NP][4] = { { 0, 1, -1, -1 }, { 0, 1, 2, -1 }, { 1, -1, -1, -1 }, { 1, 2, -1, -1 }, { 2, 3, -1, -1 }, { 3, -1, -1, -1 },
                                  { 0, 3, -1, -1 }, { 4, -1, -1, -1 }, { 4, 5, -1, -1 }, { 5, -1, -1, -1 }, { 2, 4, 5, -1 }, { 0, -1, -1, -1 },
                                  { 3, 4, -1, -1 }, { 1, 5, -1, -1 }, { 0, 2, 3, 5 }, { 2, -1, -1, -1 } };
        for (int p = NP - 1; p >= 0; --p)                              // descending: a keyframe's features are not in point order
            for (int i = 0; i < 4 && sees[p][i] >= 0; ++i) {
                Feature *ft = feature(&kf[sees[p][i]]);
                points[p]->_obs[kf[sees[p][i]]._keyframe_id] = ft;
                ft->_mappoint = points[p];
                if (p % 3 == 0) feature(&kf[sees[p][i]]);
            }
        points[9]->_bad = true;
        kf[4]._bad = true;
        const int cov[NK][3] = { { 1, 2, 3 }, { 0, -1, 2 }, { 4, 1, 3 }, { 4, 5, 0 }, { 5, 3, 2 }, { 4, 3, 1 } };    // -1: a null entry
        for (int k = 0; k < NK; ++k)
            for (int j = 0; j < 3; ++j) { kf[k]._cov_keyframes.push_back(cov[k][j] < 0 ? nullptr : &kf[cov[k][j]]); kf[k]._cov_weights.push_back(9 - j); }
        // the frames: -1 a feature without a point
        const int on[NF][8] = { { 0, -1, 2, 11, -2, -2, -2, -2 }, { 11, 2, -1, -1, 0, -2, -2, -2 }, { 8, 9, 8, -1, 7, 5, -2, -2 }, { -1, -1, -1, -2, -2, -2, -2, -2 } };
        for (int f = 0; f < NF; ++f)
            for (int j = 0; j < 8 && on[f][j] > -2; ++j) {
                Feature *ft = feature(&fr[f]);
                if (on[f][j] >= 0) ft->_mappoint = points[on[f][j]];
            }
    }
    ~World()
    {
        for (Feature *f : features) delete f;
        for (MapPoint *p : points) delete p;
        for (Frame &k : kf) k._features.clear();
        for (Frame &f : fr) f._features.clear();
    }
    Feature *feature(Frame *owner)
    {
        Feature *f = new Feature(Vector2d(3.0 * features.size(), 5.0), 0);
        f->_frame = owner;
        owner->_features.push_back(f);
        features.push_back(f);
        return f;
    }
    // everything a selection could move, except the frames' _ref_keyframe
    std::string state() const
    {
        std::ostringstream s;
        for (const Feature *f : features)
            s << (f->_mappoint ? (long)f->_mappoint->_id : -1L) << ' ' << f->_bad << ' ' << f->_depth << ' ' << f->_level << ' ' << (f->_frame ? (long)f->_frame->_id : -1L) << ';';
        for (const MapPoint *p : points) {
            s << p->_bad << ' ' << p->_cnt_visible << ' ' << p->_cnt_found << ' ' << p->_track_in_view << ' ' << p->_first_seen << ' ' << p->_last_seen << ':';
            for (const auto &ob : p->_obs) s << ob.first << ',';
            s << ';';
        }
        for (int k = 0; k < NK + NF; ++k) {
            const Frame &f = k < NK ? kf[k] : fr[k - NK];
            s << f._bad << ' ' << f._is_keyframe << ' ' << f._keyframe_id << ' ' << f._features.size() << ' ' << f._cov_keyframes.size() << ' '
              << f._connected_keyframe_weights.size() << ' ' << f._hip_slot << ' ';
            if (k < NK) s << (f._ref_keyframe ? (long)f._ref_keyframe->_keyframe_id : -1L);
            for (int i = 0; i < 7; ++i) { double T[7]; f._TCW.to7(T); s << ' ' << T[i]; }
            s << ';';
        }
        return s.str();
    }
};

vector<long> ids(const vector<Frame *> &l) { vector<long> v; for (const Frame *f : l) v.push_back((long)f->_keyframe_id); return v; }
vector<long> ids(const vector<MapPoint *> &l) { vector<long> v; for (const MapPoint *p : l) v.push_back((long)p->_id); return v; }

// DESIGN.md section 28's set: keyframes in the given order, features by index, each good point once
vector<MapPoint *> set_rule(const vector<Frame *> &list)
{
    vector<MapPoint *> out;
    std::set<const MapPoint *> seen;
    for (const Frame *kf : list)
        for (const Feature *ft : kf->_features)
            if (ft && ft->_mappoint && !ft->_mappoint->_bad && seen.insert(ft->_mappoint).second) out.push_back(ft->_mappoint);
    return out;
}
}

int main(int argc, char **argv)
{
    if (argc != 2 || strcmp(argv[1], "run") != 0) { fprintf(stderr, "usage: lms_surface run\n"); return 2; }
    World a, b;
    // the host route, frame by frame
    StereoTracker tracker;
    vector<vector<Frame *>> old_lists(NF);
    vector<int> old_ret(NF);
    for (int f = 0; f < NF; ++f) old_ret[f] = tracker.LocalKeyFrames(&a.fr[f], &old_lists[f]);
    // one call
    const std::string before = b.state();
    LocalMapSelector selector;
    vector<LocalMapSelector::Result> res;
    vector<Frame *> frames;
    for (int f = 0; f < NF; ++f) frames.push_back(&b.fr[f]);
    const int ret = selector.Select(frames, &res);
    check("call_answers_every_frame", res.size() == (size_t)NF);
    if (res.size() != (size_t)NF) return g_failed;
    check("return_value", ret == 3 && old_ret[0] > 0 && old_ret[1] > 0 && old_ret[2] > 0 && old_ret[3] == 0);
    bool lists = true, refs = true, sets = true, priors = true, voters = true;
    for (int f = 0; f < NF; ++f) {
        lists = lists && res[f].keyframes && ids(*res[f].keyframes) == ids(old_lists[f]);
        const Frame *ra = a.fr[f]._ref_keyframe, *rb = b.fr[f]._ref_keyframe;
        refs = refs && (ra != nullptr) == (rb != nullptr) && (!ra || ra->_keyframe_id == rb->_keyframe_id) && res[f].ref == rb;
        sets = sets && res[f].points && res[f].keyframes && *res[f].points == set_rule(*res[f].keyframes) && res[f].cut == 0;
        priors = priors && res[f].prior.size() == b.fr[f]._features.size();
        for (size_t j = 0; priors && j < res[f].prior.size(); ++j) {
            const MapPoint *mp = b.fr[f]._features[j]->_mappoint;
            const int at = res[f].prior[j];
            int want = -1;                                              // a point whose only observers are bad keyframes is in no set
            for (size_t i = 0; mp && i < res[f].points->size(); ++i)
                if ((*res[f].points)[i] == mp) want = (int)i;
            priors = at == want && (want >= 0 || !mp || mp->_bad || mp == b.points[7]);
        }
        int n = 0;
        for (const Frame *kf : old_lists[f]) {                         // the voters stand first: a voter sees a good point of the frame
            bool votes = false;
            for (const Feature *ft : a.fr[f]._features)
                votes = votes || (ft->_mappoint && !ft->_mappoint->_bad && ft->_mappoint->_obs.count(kf->_keyframe_id));
            n += votes;
        }
        voters = voters && res[f].voters == n;
    }
    check("lists_equal_keyframe_by_keyframe", lists);
    check("ref_keyframe_equal", refs);
    check("points_equal_the_set_rule", sets);
    check("prior_is_the_position_in_the_set", priors);
    check("voters_counted", voters);
    // the map is about something: the lists are the ones its construction forces
    check("list_of_frame_0", ids(old_lists[0]) == vector<long>({ 20, 21, 22 }) && a.fr[0]._ref_keyframe == &a.kf[0]);
    check("bad_keyframe_is_ref_and_not_listed", a.fr[2]._ref_keyframe == &a.kf[4] && ids(old_lists[2]) == vector<long>({ 23, 25, 20, 21 }));
    check("frame_without_points", res[3].keyframes && res[3].keyframes->empty() && res[3].points->empty() && res[3].ref == nullptr &&
                                  b.fr[3]._ref_keyframe == nullptr && res[3].voters == 0);
    check("equal_lists_share_one_object", res[0].keyframes == res[1].keyframes && res[0].points == res[1].points &&
                                          res[0].keyframes != res[2].keyframes && res[0].points != res[2].points);
    check("bad_point_is_in_no_set", [&] { for (int f = 0; f < NF; ++f) for (const MapPoint *p : *res[f].points) if (p->_bad) return false; return true; }());
    check("nothing_else_moves", b.state() == before);
    const LocalMapSelector::Stats &st = selector.GetStats();
    check("stats", st.frames == NF && st.keyframes == NK && st.points == NP - 1 && st.dropped == 0 && st.lists == 3 && st.observations > 0);
    // a second call forgets the first; a single-frame call answers what its batch entry did
    vector<LocalMapSelector::Result> one;
    const vector<long> kept = ids(*res[2].keyframes), kept_points = ids(*res[2].points);
    const int ret1 = selector.Select({ &b.fr[2] }, &one);
    check("single_frame_call_equals_its_batch_entry", ret1 == 1 && one.size() == 1 && ids(*one[0].keyframes) == kept && ids(*one[0].points) == kept_points);
    // failures: cleared results, 0
    vector<LocalMapSelector::Result> none(2);
    check("no_frame_fails", selector.Select({}, &none) == 0 && none.empty());
    none.resize(2);
    check("null_frame_fails", selector.Select({ &b.fr[0], nullptr }, &none) == 0 && none.empty());
    LocalMapSelector::Options o;
    o._neighbours = 33;
    LocalMapSelector wide(o);
    none.resize(2);
    check("too_many_neighbours_fails", wide.Select(frames, &none) == 0 && none.empty());
    // an observation whose feature does not point back is dropped and counted
    World c;
    c.points[0]->_obs[c.kf[1]._keyframe_id]->_mappoint = nullptr;
    vector<Frame *> cf;
    for (int f = 0; f < NF; ++f) cf.push_back(&c.fr[f]);
    vector<LocalMapSelector::Result> cr;
    LocalMapSelector sel_c;
    sel_c.Select(cf, &cr);
    check("dangling_observation_dropped", cr.size() == (size_t)NF && sel_c.GetStats().dropped == 1 && ids(*cr[0].keyframes) == vector<long>({ 20, 21, 22 }));
    return g_failed;
}
