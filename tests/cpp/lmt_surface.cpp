// ygz::LocalMapTracker against LocalMapSelector::Select followed by StereoLocalMap::TrackLocalMap, and the check lists of the two C entry
// points under it, written against include/ygz only.
//   lmt_surface check   no device: with a null context walks the check lists of ygz_hip_map_point_attributes and
//                       ygz_hip_stereo_local_map_indexed in the header's order; a refused call writes nothing
//   lmt_surface run     the map of tests/cpp/lms_surface.cpp built twice by hand -- six keyframes (ids 20 .. 25, keyframe 24 bad) with their
//                       covisible lists, sixteen map points (one bad), four tracked frames -- with what tracking needs added: QVGA pictures,
//                       poses, positions, descriptors, depths; plus point 16 whose reference observation has no descriptor and one observation
//                       whose feature does not point back.  Point 7, which lms_surface.cpp lets only the bad keyframe see, is also seen by
//                       keyframe 25 here: StereoLocalMap::TrackLocalMap refuses a frame that carries a point no set holds.  On copy A
//                       Select then TrackLocalMap run, on copy B ONE LocalMapTracker::Track.
// Each check prints "<name> ok" or "<name> FAILED"; the program exits with the number of failed checks; without an argument it prints its
// usage.  Built by tests/test_lmt_surface_build.py, run by it (check) and by tests/test_gpu_lmt_surface.py (run).
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include "ygz_hip.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <sstream>
using namespace ygz;

namespace {
int g_failed = 0;
void check(const char *name, bool ok)
{
    printf("%s %s\n", name, ok ? "ok" : "FAILED");
    if (!ok) ++g_failed;
}

const int NK = 6, NF = 4, NP = 17, W = 320, H = 240;

std::string bits(double v) { uint64_t u; memcpy(&u, &v, 8); std::ostringstream s; s << std::hex << u; return s.str(); }

struct World {
    Frame kf[NK], fr[NF];
    vector<Feature *> features;
    vector<MapPoint *> points;
    vector<uint8_t> img[NF];
    World()
    {
        for (int k = 0; k < NK; ++k) {
            kf[k]._keyframe_id = kf[k]._id = 20 + k; kf[k]._is_keyframe = true;
            const double T[7] = { 0, 0, 0, 1, 0.05 * k - 0.1, 0.02 * k, 0.03 * k };
            kf[k]._TCW = SE3::from7(T);
        }
        for (int f = 0; f < NF; ++f) {
            fr[f]._id = 100 + f;
            img[f].resize((size_t)W * H);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) img[f][(size_t)y * W + x] = (uint8_t)(((x + 3 * f) * 7 + y * 13 + ((x / 5 + y / 3) % 2) * 90 + (x * y) % 31) & 255);
            fr[f]._color = cv::Mat(H, W, CV_8UC1, img[f].data());
            fr[f].InitFrame();
            const double T[7] = { 0, 0, 0, 1, 0.01 * f, -0.01 * f, 0.0 };
            fr[f]._TCW = SE3::from7(T);
        }
        for (int p = 0; p < NP; ++p) {
            MapPoint *mp = new MapPoint;
            mp->_id = 500 + p;
            mp->_pos_world = Vector3d(0.15 * p - 1.1, 0.07 * p - 0.5, 4.0 + 0.11 * p);
            mp->_cnt_visible = mp->_cnt_found = 1;
            points.push_back(mp);
        }
        // which keyframes see which point, in feature order per keyframe: a gap feature without a point after every third
        const int sees[NP][4] = { { 0, 1, -1, -1 }, { 0, 1, 2, -1 }, { 1, -1, -1, -1 }, { 1, 2, -1, -1 }, { 2, 3, -1, -1 }, { 3, -1, -1, -1 },
                                  { 0, 3, -1, -1 }, { 4, 5, -1, -1 }, { 4, 5, -1, -1 }, { 5, -1, -1, -1 }, { 2, 4, 5, -1 }, { 0, -1, -1, -1 },
                                  { 3, 4, -1, -1 }, { 1, 5, -1, -1 }, { 0, 2, 3, 5 }, { 2, -1, -1, -1 }, { 0, 2, -1, -1 } };
        for (int p = NP - 1; p >= 0; --p)                              // descending: a keyframe's features are not in point order
            for (int i = 0; i < 4 && sees[p][i] >= 0; ++i) {
                Feature *ft = feature(&kf[sees[p][i]]);
                points[p]->_obs[kf[sees[p][i]]._keyframe_id] = ft;
                ft->_mappoint = points[p];
                ft->_level = (p + i) % 3;
                if (p % 3 == 0) feature(&kf[sees[p][i]]);
            }
        points[9]->_bad = true;
        kf[4]._bad = true;
        points[16]->_obs[kf[0]._keyframe_id]->_desc = Mat();          // the reference observation of point 16 has no descriptor
        points[0]->_obs[kf[1]._keyframe_id]->_mappoint = nullptr;      // an observation whose feature does not point back
        const int cov[NK][3] = { { 1, 2, 3 }, { 0, -1, 2 }, { 4, 1, 3 }, { 4, 5, 0 }, { 5, 3, 2 }, { 4, 3, 1 } };    // -1: a null entry
        for (int k = 0; k < NK; ++k)
            for (int j = 0; j < 3; ++j) { kf[k]._cov_keyframes.push_back(cov[k][j] < 0 ? nullptr : &kf[cov[k][j]]); kf[k]._cov_weights.push_back(9 - j); }
        // the frames: -1 a feature without a point
        const int on[NF][8] = { { 0, -1, 2, 11, -2, -2, -2, -2 }, { 11, 2, -1, -1, 0, -2, -2, -2 }, { 8, 9, 8, -1, 7, 5, -2, -2 }, { -1, -1, -1, -2, -2, -2, -2, -2 } };
        for (int f = 0; f < NF; ++f)
            for (int j = 0; j < 8 && on[f][j] > -2; ++j) {
                Feature *ft = feature(&fr[f]);
                ft->_depth = j % 2 ? 4.0 + 0.3 * j : -1.0;
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
        const size_t i = features.size();
        Feature *f = new Feature(Vector2d(40.0 + 8.0 * (double)(i % 30), 40.0 + 9.0 * (double)(i / 30)), 0);
        f->_frame = owner;
        for (int b = 0; b < 32; ++b) f->_desc.data[b] = (uint8_t)((i * 37 + (size_t)b * 11 + (i >> 2)) & 255);
        owner->_features.push_back(f);
        features.push_back(f);
        return f;
    }
    // everything selection and tracking could move; doubles by their bits.  with_frames = false: the keyframes, their features and nothing of
    // the tracked frames
    std::string state(bool with_frames) const
    {
        std::ostringstream s;
        for (const Feature *f : features) {
            const bool on_kf = f->_frame >= &kf[0] && f->_frame < &kf[NK];
            if (!with_frames && !on_kf) continue;
            s << (f->_mappoint ? (long)f->_mappoint->_id : -1L) << ' ' << f->_bad << ' ' << bits(f->_depth) << ' ' << f->_level << ' ' << (long)f->_frame->_id << ';';
        }
        for (const MapPoint *p : points) {
            s << p->_bad << ' ';
            if (with_frames) s << p->_cnt_visible << ' ' << p->_cnt_found << ' ' << p->_track_in_view << ' ';
            s << p->_first_seen << ' ' << p->_last_seen << ' ' << bits(p->_pos_world[0]) << ':';
            for (const auto &ob : p->_obs) s << ob.first << ',';
            s << ';';
        }
        for (int k = 0; k < (with_frames ? NK + NF : NK); ++k) {
            const Frame &f = k < NK ? kf[k] : fr[k - NK];
            s << f._bad << ' ' << f._is_keyframe << ' ' << f._keyframe_id << ' ' << f._features.size() << ' ' << f._cov_keyframes.size() << ' '
              << (f._ref_keyframe ? (long)f._ref_keyframe->_keyframe_id : -1L);
            double T[7];
            f._TCW.to7(T);
            for (int i = 0; i < 7; ++i) s << ' ' << bits(T[i]);
            s << ';';
        }
        return s.str();
    }
};

int run()
{
    Config::Set("image.width", "320"); Config::Set("image.height", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    World a, b;
    check("copies_start_equal", a.state(true) == b.state(true));
    // copy A: Select, then TrackLocalMap on its lists
    vector<Frame *> fa, fb;
    for (int f = 0; f < NF; ++f) { fa.push_back(&a.fr[f]); fb.push_back(&b.fr[f]); }
    LocalMapSelector selector;
    vector<LocalMapSelector::Result> sel;
    const int ret_sel = selector.Select(fa, &sel);
    check("select_answers", ret_sel > 0 && sel.size() == (size_t)NF);
    if (sel.size() != (size_t)NF) return g_failed;
    vector<const vector<Frame *> *> lists;
    for (int f = 0; f < NF; ++f) lists.push_back(sel[f].keyframes);
    StereoLocalMap slm;
    vector<StereoLocalMap::Result> old;
    const int ret_old = slm.TrackLocalMap(fa, lists, &old);
    check("host_route_answers", old.size() == (size_t)NF);
    // copy B: one Track
    const std::string kf_before = b.state(false);
    LocalMapTracker tracker;
    vector<LocalMapTracker::Result> res;
    const int ret = tracker.Track(fb, &res);
    check("track_answers_every_frame", res.size() == (size_t)NF && old.size() == (size_t)NF);
    if (res.size() != (size_t)NF || old.size() != (size_t)NF) return g_failed;
    check("return_value", ret == ret_old);
    check("state_equal_on_both_copies", a.state(true) == b.state(true));
    bool same = true, sel_same = true, moved = false;
    for (int f = 0; f < NF; ++f) {
        same = same && res[f].status == old[f].status && res[f].new_matches == old[f].new_matches && res[f].edges == old[f].edges &&
               res[f].inliers == old[f].inliers && res[f].tracked == old[f].tracked;
        sel_same = sel_same && (res[f].ref != nullptr) == (sel[f].ref != nullptr) && (!res[f].ref || res[f].ref->_keyframe_id == sel[f].ref->_keyframe_id) &&
                   res[f].voters == sel[f].voters && res[f].cut == sel[f].cut && res[f].ref == b.fr[f]._ref_keyframe;
        moved = moved || res[f].edges > 0;
    }
    check("results_equal", same);
    check("ref_voters_cut_equal", sel_same);
    check("the_case_is_about_something", moved && b.fr[0]._ref_keyframe == &b.kf[0] && b.fr[3]._ref_keyframe == nullptr);
    // the attributes the class sent, against Matcher::PointAttributes point by point
    const LocalMapTracker::Sent &sent = tracker.GetSent();
    bool attrs = sent.points.size() == (size_t)NP - 1, nodesc = false;
    for (size_t i = 0; attrs && i < sent.points.size(); ++i) {
        Matcher::PointAttr at;
        const bool usable = Matcher::PointAttributes(sent.points[i], at), ours = sent.state[i] == 1 && sent.has_desc[i];
        attrs = usable == ours;
        if (usable && ours)
            attrs = bits(at.dmax) == bits(sent.dmax[i]) && bits(at.normal[0]) == bits(sent.normal[3 * i]) && bits(at.normal[1]) == bits(sent.normal[3 * i + 1]) &&
                    bits(at.normal[2]) == bits(sent.normal[3 * i + 2]);
        if (sent.points[i] == b.points[16]) nodesc = sent.state[i] == 1 && !sent.has_desc[i];
    }
    check("attributes_bit_equal_to_point_attributes", attrs);
    const LocalMapTracker::Stats &st = tracker.GetStats();
    int in_list = 0;
    for (int f = 0; f < NF; ++f) in_list += (int)sel[f].points->size();
    int held = 0;
    for (int f = 0; f < NF; ++f) held += res[f].points;
    check("descriptorless_point_is_in_no_list_and_counted", nodesc && st.refused == 1 && st.removed >= 1 && held == in_list - st.removed);
    check("stats", st.frames == NF && st.keyframes == NK && st.points == NP - 1 && st.dropped == 1 && st.centres == NK && st.attribute_rows > st.observations);
    check("keyframes_do_not_move", b.state(false) == kf_before);
    // failures: cleared results, 0
    vector<LocalMapTracker::Result> none(2);
    check("no_frame_fails", tracker.Track({}, &none) == 0 && none.empty());
    none.resize(2);
    check("null_frame_fails", tracker.Track({ &b.fr[0], nullptr }, &none) == 0 && none.empty());
    none.resize(2);
    check("repeated_frame_fails", tracker.Track({ &b.fr[0], &b.fr[0] }, &none) == 0 && none.empty());
    return g_failed;
}

// ---- the check lists with a null context
int mpa(int K, int P, const double *c, const double *pw, const int32_t *off, const int32_t *kf, const int32_t *lv, bool outputs = true)
{
    double dmax[4] = { 5, 5, 5, 5 }, normal[12];
    int32_t state[4] = { 5, 5, 5, 5 };
    for (double &v : normal) v = 5;
    const int rc = ygz_hip_map_point_attributes(nullptr, K, c, P, pw, off, kf, lv, outputs ? dmax : nullptr, normal, state);
    bool clean = true;
    for (int i = 0; i < 4; ++i) clean = clean && dmax[i] == 5 && state[i] == 5 && normal[3 * i] == 5;
    return clean ? rc : -1000;
}

struct Idx {
    int P = 3, n_lists = 1, stride = 4, F = 1;
    double pw[9] = { 1, 1, 1, 2, 2, 2, 3, 3, 3 }, dmax[3] = { 1, 2, 3 }, normal[9] = { 0, 0, 1, 0, 0, 1, 0, 0, 1 }, T[7] = { 0, 0, 0, 1, 0, 0, 0 };
    uint8_t desc[96] = { 0 };
    int32_t lists[4] = { 0, 1, 2, 0 }, len[1] = { 3 }, slot[1] = { 0 }, li[1] = { 0 };
    const double *p_pw = pw, *p_T = T;
    const int32_t *p_lists = lists, *p_len = len;
    ygz_slm_params prm;
    bool with_prm = false, with_out = true;
    int call()
    {
        double T_out[7] = { 5, 5, 5, 5, 5, 5, 5 };
        int32_t status[1] = { 5 }, counts[8] = { 5, 5, 5, 5, 5, 5, 5, 5 };
        const int rc = ygz_hip_stereo_local_map_indexed(nullptr, P, p_pw, desc, dmax, normal, n_lists, stride, p_lists, p_len, F, slot, li, p_T, nullptr,
                                                        with_prm ? &prm : nullptr, with_out ? T_out : nullptr, status, counts, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                        nullptr, nullptr, nullptr, nullptr);
        return T_out[0] == 5 && T_out[6] == 5 && status[0] == 5 && counts[0] == 5 && counts[7] == 5 ? rc : -1000;
    }
};

int walk()
{
    const int INV = YGZ_E_INVALID, CAP = YGZ_E_CAPACITY;
    const double c[6] = { 0, 0, 0, 1, 1, 1 }, pw[6] = { 0, 0, 3, 1, 0, 4 }, inf = std::numeric_limits<double>::infinity();
    const int32_t off[3] = { 0, 2, 3 }, kf[3] = { 0, 1, 1 }, lv[3] = { 0, 1, -2 };
    check("mpa_valid_call_wants_a_context", mpa(2, 2, c, pw, off, kf, lv) == INV);
    check("mpa_nulls_and_counts", mpa(2, 2, nullptr, pw, off, kf, lv) == INV && mpa(2, 2, c, nullptr, off, kf, lv) == INV && mpa(2, 2, c, pw, nullptr, kf, lv) == INV &&
                                  mpa(2, 2, c, pw, off, nullptr, lv) == INV && mpa(2, 2, c, pw, off, kf, nullptr) == INV && mpa(2, 2, c, pw, off, kf, lv, false) == INV &&
                                  mpa(0, 2, c, pw, off, kf, lv) == INV && mpa(2, 0, c, pw, off, kf, lv) == INV);
    const int32_t bad_off[3] = { 1, 2, 3 }, dec_off[3] = { 0, 3, 2 };
    check("mpa_capacity_before_offsets", mpa(YGZ_MAP_MAX_KEYFRAMES + 1, 2, c, pw, bad_off, kf, lv) == CAP && mpa(2, YGZ_MPA_MAX_POINTS + 1, c, pw, bad_off, kf, lv) == CAP &&
                                         mpa(YGZ_MAP_MAX_KEYFRAMES + 1, 2, c, pw, off, kf, lv, false) == INV);
    check("mpa_offsets", mpa(2, 2, c, pw, bad_off, kf, lv) == INV && mpa(2, 2, c, pw, dec_off, kf, lv) == INV);
    const int32_t long_off[3] = { 0, YGZ_MAP_MAX_OBS_PER_POINT + 1, YGZ_MAP_MAX_OBS_PER_POINT + 1 }, out_kf[3] = { 0, 2, 1 }, neg_kf[3] = { -1, 1, 1 }, hi_lv[3] = { 0, 31, 0 };
    check("mpa_rows_before_the_rows_are_read", mpa(2, 2, c, pw, long_off, out_kf, lv) == CAP);
    const double nan_c[6] = { 0, std::nan(""), 0, 1, 1, 1 }, inf_pw[6] = { 0, 0, 3, inf, 0, 4 };
    check("mpa_indices_levels_finiteness", mpa(2, 2, c, pw, off, out_kf, lv) == INV && mpa(2, 2, c, pw, off, neg_kf, lv) == INV && mpa(2, 2, c, pw, off, kf, hi_lv) == INV &&
                                           mpa(2, 2, nan_c, pw, off, kf, lv) == INV && mpa(2, 2, c, inf_pw, off, kf, lv) == INV);
    {
        Idx v;
        check("indexed_valid_call_wants_a_context", v.call() == INV);
        Idx a1; a1.p_lists = nullptr; Idx a2; a2.p_len = nullptr; Idx a3; a3.p_T = nullptr; Idx a4; a4.with_out = false; Idx a5; a5.F = 0; Idx a6; a6.n_lists = 0; Idx a7; a7.P = -1;
        check("indexed_nulls_and_counts", a1.call() == INV && a2.call() == INV && a3.call() == INV && a4.call() == INV && a5.call() == INV && a6.call() == INV && a7.call() == INV);
        Idx b1; b1.F = YGZ_SLM_MAX_FRAMES + 1; Idx b2; b2.n_lists = YGZ_SLM_MAX_FRAMES + 1; Idx b3; b3.P = YGZ_MPA_MAX_POINTS + 1;
        Idx b4; b4.F = YGZ_SLM_MAX_FRAMES + 1; ygz_hip_default_slm_params(&b4.prm); b4.prm.th = 0; b4.with_prm = true;
        Idx b5; b5.F = YGZ_SLM_MAX_FRAMES + 1; b5.p_T = nullptr;
        check("indexed_capacity_before_parameters", b1.call() == CAP && b2.call() == CAP && b3.call() == CAP && b4.call() == CAP && b5.call() == INV);
        Idx c1; ygz_hip_default_slm_params(&c1.prm); c1.prm.ratio = -1; c1.with_prm = true; Idx c2; ygz_hip_default_slm_params(&c2.prm); c2.prm.th_dist = 257; c2.with_prm = true;
        check("indexed_parameters", c1.call() == INV && c2.call() == INV);
        Idx d1; d1.p_pw = nullptr; Idx d2; d2.stride = 0; Idx d3; d3.len[0] = 5; Idx d4; d4.len[0] = -1; Idx d5; d5.slot[0] = -1; Idx d6; d6.li[0] = 1; Idx d7; d7.lists[1] = 3;
        Idx d8; d8.lists[2] = -1; Idx d9; d9.lists[3] = 99;
        check("indexed_map_and_lists", d1.call() == INV && d2.call() == INV && d3.call() == INV && d4.call() == INV && d5.call() == INV && d6.call() == INV &&
                                       d7.call() == INV && d8.call() == INV && d9.call() == INV);
        Idx e1; e1.T[4] = inf; Idx e2; e2.pw[7] = std::nan(""); e2.lists[2] = 0; Idx e3; e3.dmax[1] = inf; Idx e4; e4.normal[8] = std::nan("");
        check("indexed_finiteness_over_the_whole_map", e1.call() == INV && e2.call() == INV && e3.call() == INV && e4.call() == INV);
    }
    return g_failed;
}
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "check") == 0) return walk();
    if (argc == 2 && strcmp(argv[1], "run") == 0) return run();
    fprintf(stderr, "usage: lmt_surface check | run\n");
    return 2;
}
