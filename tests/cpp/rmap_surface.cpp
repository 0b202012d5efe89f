// ygz::ResidentMap against ygz::LocalMapTracker, and the check lists of the C entry points under it, written against include/ygz only.
//   rmap_surface check  no device: with a null context walks the check lists of ygz_hip_map_upload, ygz_hip_map_update and
//                       ygz_hip_stereo_local_map_resident in the header's order; a refused call writes nothing
//   rmap_surface run    the map of tests/cpp/lmt_surface.cpp built twice.  On copy A ONE LocalMapTracker::Track runs, on copy B
//                       ResidentMap::Upload of the six keyframes and ONE ResidentMap::Track: _TCW bitwise, every feature, every point counter,
//                       _ref_keyframe and the results are equal.  Then on two more copies three points and one keyframe move: one copy goes
//                       through Upload (before the move), Update and Track, the other through a fresh Upload and Track, and both end equal.
// Each check prints "<name> ok" or "<name> FAILED"; the program exits with the number of failed checks; without an argument it prints its
// usage.  Built by tests/test_rmap_surface_build.py, run by it (check) and by tests/test_gpu_rmap_surface.py (run).
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

vector<Frame *> frames_of(World &w) { vector<Frame *> v; for (int f = 0; f < NF; ++f) v.push_back(&w.fr[f]); return v; }
vector<Frame *> keyframes_of(World &w) { vector<Frame *> v; for (int k = NK - 1; k >= 0; --k) v.push_back(&w.kf[k]); v.push_back(nullptr); v.push_back(&w.kf[2]); return v; }

bool results_equal(const vector<LocalMapTracker::Result> &x, const vector<LocalMapTracker::Result> &y)
{
    bool same = x.size() == y.size();
    for (size_t f = 0; same && f < x.size(); ++f)
        same = x[f].status == y[f].status && x[f].new_matches == y[f].new_matches && x[f].edges == y[f].edges && x[f].inliers == y[f].inliers &&
               x[f].tracked == y[f].tracked && (x[f].ref != nullptr) == (y[f].ref != nullptr) &&
               (!x[f].ref || x[f].ref->_keyframe_id == y[f].ref->_keyframe_id) && x[f].voters == y[f].voters && x[f].cut == y[f].cut &&
               x[f].points == y[f].points;
    return same;
}

// what a bundle adjustment leaves: three points and one keyframe somewhere else, one point bad
void move(World &w)
{
    w.points[1]->_pos_world += Vector3d(0.02, -0.01, 0.03);
    w.points[4]->_pos_world += Vector3d(-0.01, 0.02, 0.01);
    w.points[14]->_pos_world += Vector3d(0.0, 0.01, -0.02);
    const double T[7] = { 0, 0, 0, 1, -0.07, 0.03, 0.05 };
    w.kf[2]._TCW = SE3::from7(T);
    w.points[11]->_bad = true;
}

int run()
{
    Config::Set("image.width", "320"); Config::Set("image.height", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    {
        World a, b;
        check("copies_start_equal", a.state(true) == b.state(true));
        vector<Frame *> fa = frames_of(a), fb = frames_of(b);
        LocalMapTracker tracker;
        vector<LocalMapTracker::Result> old, res;
        const int ret_old = tracker.Track(fa, &old);
        check("tracker_answers", old.size() == (size_t)NF);
        ResidentMap rm;
        vector<ResidentMap::Result> none(2);
        check("track_before_upload_fails", rm.Track(fb, &none) == 0 && none.empty() && !rm.Resident());
        const std::string kf_before = b.state(false);
        check("upload", rm.Upload(keyframes_of(b)) && rm.Resident());
        const int ret = rm.Track(fb, &res);
        check("track_answers_every_frame", res.size() == (size_t)NF);
        if (res.size() != (size_t)NF || old.size() != (size_t)NF) return g_failed + 1;
        check("return_value", ret == ret_old);
        check("state_equal_on_both_copies", a.state(true) == b.state(true));
        check("results_equal", results_equal(old, res));
        bool moved = false;
        for (int f = 0; f < NF; ++f) moved = moved || res[f].edges > 0;
        check("the_case_is_about_something", moved && b.fr[0]._ref_keyframe == &b.kf[0] && b.fr[3]._ref_keyframe == nullptr);
        const ResidentMap::Stats &st = rm.GetStats();
        const LocalMapTracker::Stats &lt = tracker.GetStats();
        check("stats", st.keyframes == NK && st.points == lt.points && st.observations == lt.observations && st.dropped == lt.dropped &&
                       st.centres == lt.centres && st.attribute_rows == lt.attribute_rows && st.refused == lt.refused && st.removed == lt.removed &&
                       st.uploads == 1 && st.updates == 0 && st.frames == NF && st.unknown == 0);
        check("keyframes_do_not_move", b.state(false) == kf_before);
        none.resize(2);
        check("no_frame_fails", rm.Track({}, &none) == 0 && none.empty());
        none.resize(2);
        check("null_frame_fails", rm.Track({ &b.fr[0], nullptr }, &none) == 0 && none.empty());
        none.resize(2);
        check("repeated_frame_fails", rm.Track({ &b.fr[0], &b.fr[0] }, &none) == 0 && none.empty());
        check("upload_of_nothing_fails_and_keeps_the_map", !rm.Upload({}) && !rm.Upload({ nullptr }) && rm.Resident() && rm.GetStats().uploads == 1);
    }
    {
        World c, d;
        vector<Frame *> fc = frames_of(c), fd = frames_of(d);
        ResidentMap rc, rd;
        check("upload_before_the_move", rc.Upload(keyframes_of(c)));
        move(c); move(d);
        MapPoint stranger;
        Frame outsider;
        const int pushed = rc.Update({ c.points[1], c.points[4], c.points[14], c.points[11], &stranger, c.points[4] }, { &c.kf[2], &outsider });
        check("update_pushes_and_skips", pushed == 5 && rc.GetStats().skipped == 2 && rc.GetStats().updates == 1);
        check("fresh_upload_after_the_move", rd.Upload(keyframes_of(d)));
        vector<ResidentMap::Result> ru, rf;
        const int tu = rc.Track(fc, &ru), tf = rd.Track(fd, &rf);
        check("update_then_track_equals_upload_then_track", tu == tf && ru.size() == (size_t)NF && results_equal(ru, rf) && c.state(true) == d.state(true));
        bool about = false;
        for (size_t f = 0; f < ru.size(); ++f) about = about || ru[f].edges > 0;
        check("the_update_case_is_about_something", about);
    }
    return g_failed;
}

// ---- the check lists with a null context
struct Small {
    uint8_t kf_bad[2] = { 0, 0 }, desc[96] = { 0 };
    int32_t cov[2] = { 1, -1 }, off[4] = { 0, 2, 2, 3 }, kf[3] = { 0, 1, 1 }, feat[3] = { 5, 0, 7 };
    double centre[6] = { 0, 0, 0, 1, 0, 0 }, pw[9] = { 0, 0, 4, 1, 0, 4, 2, 0, 4 };
    int32_t a_off[4] = { 0, 1, 3, 3 }, a_kf[3] = { 1, 0, 0 }, a_lv[3] = { 0, 30, -2 };
    ygz_map_arrays m;
    Small()
    {
        memset(&m, 0, sizeof m);
        m.n_keyframes = 2; m.n_cov = 1; m.n_points = 3; m.n_centres = 2;
        m.kf_bad = kf_bad; m.cov = cov; m.offsets = off; m.kf = kf; m.feat = feat;
        m.centre = centre; m.a_offsets = a_off; m.a_kf = a_kf; m.a_level = a_lv; m.pw = pw; m.pt_desc = desc;
    }
    int call()
    {
        double dmax[3] = { 5, 5, 5 }, normal[9] = { 5, 5, 5, 5, 5, 5, 5, 5, 5 };
        int32_t state[3] = { 5, 5, 5 };
        const int rc = ygz_hip_map_upload(nullptr, nullptr, &m, dmax, normal, state);
        return dmax[0] == 5 && dmax[2] == 5 && normal[8] == 5 && state[1] == 5 ? rc : -1000;
    }
};

struct Res {
    int F = 1;
    int32_t slot[1] = { 0 }, fr_off[3] = { 0, 2, 2 }, fr_pt[2] = { 0, -1 };
    double T[7] = { 0, 0, 0, 1, 0, 0, 0 };
    const int32_t *p_slot = slot, *p_off = fr_off, *p_pt = fr_pt;
    const double *p_T = T;
    ygz_lms_params q;
    bool with_q = false, with_out = true;
    Res() { ygz_hip_default_lms_params(&q); }
    int call()
    {
        double T_out[7] = { 5, 5, 5, 5, 5, 5, 5 };
        int32_t n_pt[2] = { 5, 5 }, status[2] = { 5, 5 };
        const int rc = ygz_hip_stereo_local_map_resident(nullptr, nullptr, F, p_slot, p_T, p_off, p_pt, with_q ? &q : nullptr, nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, nullptr, nullptr, n_pt, nullptr, nullptr, nullptr, with_out ? T_out : nullptr,
                                                         status, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        return T_out[0] == 5 && T_out[6] == 5 && n_pt[0] == 5 && status[0] == 5 ? rc : -1000;
    }
};

int walk()
{
    const int INV = YGZ_E_INVALID, CAP = YGZ_E_CAPACITY;
    ygz_hip_map *m = nullptr;
    ygz_map_info info;
    memset(&info, 5, sizeof info);
    check("object_calls_want_a_context", ygz_hip_map_create(nullptr, &m) == INV && m == nullptr && ygz_hip_map_destroy(nullptr, nullptr) == INV &&
                                         ygz_hip_map_info(nullptr, nullptr, &info) == INV && info.uploads == 0x05050505 &&
                                         ygz_hip_map_download(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == INV);
    { Small v; check("upload_valid_call_wants_a_context", v.call() == INV && ygz_hip_map_upload(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == INV); }
    { Small a; a.m.kf_bad = nullptr; Small b; b.m.feat = nullptr; Small c; c.m.n_points = 0; Small d; d.m.n_cov = -1; Small e; e.m.cov = nullptr;
      check("upload_selection_nulls_and_counts", a.call() == INV && b.call() == INV && c.call() == INV && d.call() == INV && e.call() == INV); }
    { Small a; a.m.n_keyframes = YGZ_LMS_MAX_KEYFRAMES + 1; a.off[0] = 1; Small b; b.m.n_cov = YGZ_LMS_MAX_COV + 1; b.m.centre = nullptr;
      check("upload_selection_capacity_before_offsets_and_attributes", a.call() == CAP && b.call() == CAP); }
    { Small a; a.off[0] = 1; Small b; b.kf[0] = 1; Small c; c.feat[1] = YGZ_LMS_MAX_FEATURES; Small d; d.cov[0] = 2; Small e; e.off[0] = 1; e.m.centre = nullptr;
      check("upload_selection_arrays_before_attributes", a.call() == INV && b.call() == INV && c.call() == INV && d.call() == INV && e.call() == INV); }
    { Small a; a.m.centre = nullptr; Small b; b.m.a_kf = nullptr; Small c; c.m.n_centres = 0; Small d; d.m.n_centres = YGZ_MAP_MAX_KEYFRAMES + 1; d.a_off[0] = 1;
      Small e; e.a_off[3] = 2; Small f; f.a_kf[1] = 2; Small g; g.a_lv[0] = 31; Small h; h.pw[4] = std::nan(""); Small i; i.centre[0] = std::numeric_limits<double>::infinity();
      check("upload_attribute_side", a.call() == INV && b.call() == INV && c.call() == INV && d.call() == CAP && e.call() == INV && f.call() == INV && g.call() == INV &&
                                     h.call() == INV && i.call() == INV); }
    { Small a; a.m.pt_desc = nullptr; Small b; b.m.pt_desc = nullptr; b.pw[0] = std::nan("");
      check("upload_descriptor_last", a.call() == INV && b.call() == INV); }
    {
        const int32_t idx[1] = { 0 };
        const double x[3] = { 0, 0, 0 };
        check("update_wants_a_context_and_a_map", ygz_hip_map_update(nullptr, nullptr, 1, idx, x, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr) == INV);
    }
    { Res v; check("resident_valid_call_wants_a_context", v.call() == INV); }
    { Res a; a.p_slot = nullptr; Res b; b.p_T = nullptr; Res c; c.p_off = nullptr; Res d; d.p_pt = nullptr; Res e; e.with_out = false; Res f; f.F = 0;
      check("resident_nulls_and_counts", a.call() == INV && b.call() == INV && c.call() == INV && d.call() == INV && e.call() == INV && f.call() == INV); }
    { Res a; a.F = YGZ_LMS_MAX_FRAMES + 1; a.q.max_points = 0; a.with_q = true; Res b; b.F = YGZ_LMS_MAX_FRAMES + 1; b.p_T = nullptr;
      check("resident_capacity_before_parameters", a.call() == CAP && b.call() == INV); }
    { Res a; a.q.max_keyframes = 0; a.with_q = true; Res b; b.q.max_keyframes = YGZ_LMS_MAX_KEYFRAMES + 1; b.with_q = true; Res c; c.q.max_points = 0; c.with_q = true;
      Res d; d.q.max_points = YGZ_SLM_MAX_PAIRS + 1; d.with_q = true; Res e; e.q.max_points = YGZ_SLM_MAX_PAIRS + 1; e.with_q = true; e.fr_off[0] = 1;
      check("resident_parameters_and_pairs_before_offsets", a.call() == INV && b.call() == INV && c.call() == INV && d.call() == CAP && e.call() == CAP); }
    { Res a; a.fr_off[0] = 1; Res b; b.fr_off[1] = -1; Res c; c.fr_off[1] = YGZ_LMS_MAX_FEATURES + 1; c.fr_off[2] = c.fr_off[1];
      Res d; d.fr_pt[0] = 99;                                                // the entries are checked against the map: the context and the map come first
      check("resident_offsets_then_the_context", a.call() == INV && b.call() == INV && c.call() == CAP && d.call() == INV); }
    return g_failed;
}
}

int main(int argc, char **argv)
{
    if (argc == 2 && strcmp(argv[1], "check") == 0) return walk();
    if (argc == 2 && strcmp(argv[1], "run") == 0) return run();
    fprintf(stderr, "usage: rmap_surface check | run\n");
    return 2;
}
