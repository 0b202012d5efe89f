// ygz::LoopClosing::SearchLoopMapPoints and Matcher::SearchBySim3 / SearchByProjection / SearchFuseCandidates used the way ORB-SLAM2's
// LoopClosing::ComputeSim3 uses them, written against include/ygz only: the rendered loop scene of tests/cpp/loop_surface.cpp (an "old" run
// of keyframes, a "revisit" run in a drifted world), each revisit keyframe through DetectLoop / ComputeSim3 until a loop is accepted, then
// the widening.  The program gathers, with code of its own, the arrays each Matcher method hands to the device (the documented rules of
// Matcher.h) and keeps them with the methods' results as named blobs, which tests/widen_driver.py compares with tests/proj_ref.c.
// Built as a shared object by tests/test_proj_surface_build.py (-Wl,--no-undefined).
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <cstdio>
#include <cstring>
#include <string>
using namespace ygz;

namespace {
struct Scene {
    int w, h;
    PinholeCamera *cam;
    FeatureDetector *det;
    vector<Frame *> kfs;
    vector<MapPoint *> mps;
};

// a keyframe at true pose T_true whose map (pose and points) lives in the world D maps the true one to
Frame *make_keyframe(Scene &s, const uint8_t *bgr, const float *depth, const double *T_true7, const Sim3 &D)
{
    Frame *kf = new Frame;
    kf->_color = cv::Mat(s.h, s.w, CV_8UC3, const_cast<uint8_t *>(bgr));
    kf->InitFrame();
    const SE3 T = SE3::from7(T_true7);
    s.det->Detect(kf);
    s.det->ComputeAngleAndDescriptor(kf);
    Memory::RegisterKeyFrame(kf);
    kf->_id = kf->_keyframe_id;
    const SO3 Rp = T.so3() * D.R.inverse();
    kf->_TCW = SE3(Rp, D.s * T.translation() - Rp * D.t);
    for (Feature *f : kf->_features) {
        const double d = depth[(size_t)(int)f->_pixel[1] * s.w + (int)f->_pixel[0]];
        if (!(d > 0)) continue;
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_pos_world = D * s.cam->Pixel2World(f->_pixel, T, d);
        mp->_obs[kf->_keyframe_id] = f;
        f->_mappoint = mp; f->_depth = d * D.s;
        s.mps.push_back(mp);
    }
    kf->ComputeBoW();
    s.kfs.push_back(kf);
    return kf;
}

void link_keyframes(Frame *a, Frame *b, int w)
{
    a->AddConnection(b, w);
    b->AddConnection(a, w);
}

double map_sum(const Scene &s)
{
    double sum = 0;
    for (Frame *kf : s.kfs) {
        double t[7]; kf->_TCW.to7(t);
        for (double v : t) sum += v;
        sum += (double)kf->_features.size() + 3.0 * kf->_bow_vec.size() + 7.0 * kf->_feature_vec.size();
        for (const auto &c : kf->_connected_keyframe_weights) sum += c.second + 0.001 * c.first->_keyframe_id;
        sum += 11.0 * kf->_cov_keyframes.size();
        for (Feature *f : kf->_features) sum += f->_pixel[0] + (f->_mappoint ? 1.0 + 1e-3 * (double)f->_mappoint->_id : 0.0) + f->_level + f->_desc.data[7];
    }
    for (MapPoint *mp : s.mps) sum += mp->_pos_world[0] + mp->_pos_world[1] + mp->_pos_world[2] + mp->_obs.size() + mp->_bad + mp->_cnt_found + mp->_cnt_visible;
    return sum;
}

// ---- named blobs ----------------------------------------------------------------------------------------------------------------------
map<std::string, vector<uint8_t>> g_blobs;
template <typename T> void put(const std::string &name, const vector<T> &v)
{
    vector<uint8_t> &b = g_blobs[name];
    b.resize(v.size() * sizeof(T));
    if (!v.empty()) memcpy(b.data(), v.data(), b.size());
}

// ---- the arrays of a problem, by the rules of Matcher.h ----------------------------------------------------------------------------------
bool usable(const MapPoint *mp) { return mp != nullptr && !mp->_bad; }

struct Arrays {
    vector<double> kp_px, pw, dmax, normal, S;
    vector<int32_t> kp_level;
    vector<uint8_t> kp_desc, kp_taken, pt_desc, skip;

    void target(const Frame *kf)
    {
        for (const Feature *f : kf->_features) {
            kp_px.push_back(f->_pixel[0]); kp_px.push_back(f->_pixel[1]);
            kp_level.push_back(f->_level < 0 ? 0 : f->_level);
            for (int k = 0; k < 32; ++k) kp_desc.push_back(f->_desc.data[k]);
            kp_taken.push_back(0);
        }
    }
    void source(const MapPoint *mp, bool skipped)
    {
        // the reference observation: the lowest key with a feature and a frame; the normal: the mean of the unit rays over those observations
        const Feature *ref = nullptr;
        Vector3d sum(0, 0, 0);
        int n = 0;
        if (mp && !skipped)
            for (auto it = mp->_obs.begin(); it != mp->_obs.end(); ++it) {
                if (!it->second || !it->second->_frame) continue;
                if (!ref) ref = it->second;
                const Vector3d ray = mp->_pos_world - it->second->_frame->GetCamCenter();
                sum += ray / ray.norm();
                ++n;
            }
        const bool use = ref != nullptr;
        skip.push_back(use ? 0 : 1);
        const uint8_t *d = nullptr;
        if (use) d = (mp->_distinctive_desc.data && mp->_distinctive_desc.rows * mp->_distinctive_desc.cols == 32) ? mp->_distinctive_desc.data : ref->_desc.data;
        for (int k = 0; k < 32; ++k) pt_desc.push_back(use ? d[k] : 0);
        const Vector3d nm = use ? sum / (double)n : Vector3d(0, 0, 0);
        for (int k = 0; k < 3; ++k) { pw.push_back(use ? mp->_pos_world[k] : 0.0); normal.push_back(nm[k]); }
        dmax.push_back(use ? (mp->_pos_world - ref->_frame->GetCamCenter()).norm() * (double)(1 << (ref->_level < 0 ? 0 : ref->_level)) : 1.0);
    }
    void transform(const Sim3 &T) { S.resize(8); T.to8(S.data()); }
    void keep(const std::string &prefix, bool with_normal) const
    {
        put(prefix + "kp_px", kp_px); put(prefix + "kp_level", kp_level); put(prefix + "kp_desc", kp_desc); put(prefix + "kp_taken", kp_taken);
        put(prefix + "pw", pw); put(prefix + "pt_desc", pt_desc); put(prefix + "pt_dmax", dmax); put(prefix + "pt_skip", skip); put(prefix + "S", S);
        if (with_normal) put(prefix + "pt_normal", normal);
    }
};

Sim3 without_scale(const Sim3 &S) { return Sim3(S.R, S.t / S.s, 1.0); }
}

extern "C" {

// the blob `name`: its bytes (0 when there is none)
size_t widen_blob(const char *name, const void **data)
{
    auto it = g_blobs.find(name);
    if (it == g_blobs.end()) { *data = nullptr; return 0; }
    *data = it->second.data();
    return it->second.size();
}

// The scene of loop_run (tests/cpp/loop_surface.cpp) without the other texture's run.  out [32]:
//   0 a loop was accepted (ComputeSim3), 1 the index of that revisit keyframe, 2 matched keyframe id, 3 GetMatches size,
//   4 SearchLoopMapPoints' return, 5 sim3_added, 6 projection_added, 7 total_matches, 8 map checksum unchanged over everything,
//   9 GetCurrentMatchedPoints equals the methods called one by one, 10 GetLoopMapPoints equals the program's own collection,
//   11 SearchBySim3's return, 12 SearchByProjection's return, 13 SearchFuseCandidates' return, 14 features of the current keyframe,
//   15 loop map points, 16 keyframes of the fuse call, 17 a second SearchLoopMapPoints gives the same vector
// Returns 0, 1 on an exception, 2 when the vocabulary does not load.
int widen_run(int w, int h, const uint8_t *old_bgr, const float *old_depth, const double *old_T, int n_old, const uint8_t *lead_bgr,
              const float *lead_depth, const double *lead_T, const uint8_t *rev_bgr, const float *rev_depth, const double *rev_T, int n_rev,
              const double *drift, int min_kf_gap, int consistency_th, const void *vocab, size_t vocab_bytes, double *out)
{
    try {
        g_blobs.clear();
        for (int k = 0; k < 32; ++k) out[k] = 0;
        Config::Set("image.width", std::to_string(w)); Config::Set("image.height", std::to_string(h));
        PinholeCamera cam;
        Frame::SetCamera(&cam);
        ORBVocabulary voc;
        if (!voc.loadFromMemory(vocab, vocab_bytes)) return 2;
        Frame::SetORBVocabulary(&voc);
        FeatureDetector detector;
        detector.LoadParams();
        Memory::Clean();
        Scene s{ w, h, &cam, &detector, {}, {} };
        const size_t fb = (size_t)w * h * 3, db = (size_t)w * h;
        const Sim3 I, D = Sim3::from8(drift);
        vector<Frame *> old;
        for (int k = 0; k < n_old; ++k) old.push_back(make_keyframe(s, old_bgr + k * fb, old_depth + k * db, old_T + 7 * k, I));
        for (int i = 0; i < n_old; ++i)
            for (int j = i + 1; j < n_old && j <= i + 2; ++j) link_keyframes(old[i], old[j], 100 - 20 * (j - i));
        for (Frame *kf : old) kf->UpdateBestCovisibles();
        vector<Frame *> rev;
        rev.push_back(make_keyframe(s, lead_bgr, lead_depth, lead_T, D));
        LoopClosing lc;
        lc._option._min_kf_gap = min_kf_gap; lc._option._consistency_th = consistency_th;
        Frame *cur = nullptr;
        for (int k = 0; k < n_rev && !cur; ++k) {
            Frame *kf = make_keyframe(s, rev_bgr + k * fb, rev_depth + k * db, rev_T + 7 * k, D);
            for (Frame *r : rev) link_keyframes(kf, r, 50);
            rev.push_back(kf);
            for (Frame *r : rev) { r->_cov_keyframes.clear(); r->_cov_weights.clear(); r->UpdateBestCovisibles(); }
            if (lc.DetectLoop(kf, s.kfs) && lc.ComputeSim3()) { cur = kf; out[1] = k; }
        }
        if (cur) {
            out[0] = 1;
            Frame *loop = lc.GetMatchedKeyframe();
            const Sim3 S12 = lc.GetSim3(), Scw = lc.GetCorrectedPose();
            out[2] = (double)loop->_keyframe_id; out[3] = (double)lc.GetMatches().size();
            const double m0 = map_sum(s);
            const size_t n1 = cur->_features.size(), n2 = loop->_features.size();
            Matcher matcher;
            const Matrix3d K = cam.GetCameraMatrix();
            put("K4", vector<double>{ K(0, 0), K(1, 1), K(0, 2), K(1, 2) });

            // the seeds: GetMatches() per feature of the current keyframe
            vector<MapPoint *> seeds(n1, nullptr);
            for (const auto &m : lc.GetMatches())
                for (size_t i = 0; i < n1; ++i)
                    if (cur->_features[i]->_mappoint == m.first) seeds[i] = m.second;
            map<const MapPoint *, int> feature2;                         // map point of the loop keyframe -> its feature index
            for (size_t j = 0; j < n2; ++j) if (loop->_features[j]->_mappoint) feature2[loop->_features[j]->_mappoint] = (int)j;

            // SearchBySim3: a = the current keyframe's points into the loop keyframe, b = the other way
            Arrays a, b;
            a.target(loop); b.target(cur);
            for (size_t j = 0; j < n2; ++j) a.kp_taken[j] = usable(loop->_features[j]->_mappoint) ? 0 : 1;
            for (size_t i = 0; i < n1; ++i) b.kp_taken[i] = usable(cur->_features[i]->_mappoint) ? 0 : 1;
            std::set<const MapPoint *> seeded;
            for (MapPoint *mp : seeds) if (mp) seeded.insert(mp);
            for (size_t i = 0; i < n1; ++i) { const MapPoint *mp = cur->_features[i]->_mappoint; a.source(mp, !usable(mp) || seeds[i] != nullptr); }
            for (size_t j = 0; j < n2; ++j) { const MapPoint *mp = loop->_features[j]->_mappoint; b.source(mp, !usable(mp) || seeded.count(mp) > 0); }
            a.transform(S12.inverse() * cur->_TCW); b.transform(S12 * loop->_TCW);
            a.keep("s3a_", false); b.keep("s3b_", false);
            vector<MapPoint *> v1 = seeds;
            out[11] = matcher.SearchBySim3(cur, loop, v1, S12, 7.5f);
            vector<int32_t> r1(n1, -1);                                  // per feature of the current keyframe: -2 a seed, else the loop keyframe's feature added (-1: none)
            for (size_t i = 0; i < n1; ++i) r1[i] = seeds[i] ? -2 : (v1[i] ? feature2[v1[i]] : -1);
            put("s3_result", r1);

            // the loop map points, collected here
            vector<Frame *> group(1, loop);
            for (const auto &c : loop->_connected_keyframe_weights) if (c.first && !c.first->_bad && c.first != loop) group.push_back(c.first);
            std::sort(group.begin(), group.end(), [](const Frame *x, const Frame *y) { return x->_keyframe_id < y->_keyframe_id; });
            vector<MapPoint *> loop_points;
            std::set<MapPoint *> seen;
            for (Frame *g : group)
                for (Feature *f : g->_features)
                    if (usable(f->_mappoint) && seen.insert(f->_mappoint).second) loop_points.push_back(f->_mappoint);
            map<const MapPoint *, int> loop_index;
            for (size_t i = 0; i < loop_points.size(); ++i) loop_index[loop_points[i]] = (int)i;

            // SearchByProjection on top of SearchBySim3's vector
            Arrays p;
            p.target(cur);
            std::set<const MapPoint *> have;
            for (size_t i = 0; i < n1; ++i) if (v1[i]) { p.kp_taken[i] = 1; have.insert(v1[i]); }
            for (const MapPoint *mp : loop_points) p.source(mp, !usable(mp) || have.count(mp) > 0);
            p.transform(without_scale(Scw));
            p.keep("sp_", true);
            vector<MapPoint *> v2 = v1;
            out[12] = matcher.SearchByProjection(cur, Scw, loop_points, v2, 10.0f);
            vector<int32_t> r2(n1, -1);                                  // per feature: the loop point SearchByProjection added (-1: none)
            for (size_t i = 0; i < n1; ++i) if (v2[i] && !v1[i]) r2[i] = loop_index[v2[i]];
            put("sp_result", r2);

            // the class
            out[4] = lc.SearchLoopMapPoints();
            const LoopClosing::Stats &st = lc.GetStats();
            out[5] = st.sim3_added; out[6] = st.projection_added; out[7] = st.total_matches;
            out[9] = lc.GetCurrentMatchedPoints() == v2;
            out[10] = lc.GetLoopMapPoints() == loop_points;
            vector<int32_t> fin(n1, -1);                                 // per feature: its loop map point as an index into the loop map points
            vector<double> cur_px, loop_pw;
            for (size_t i = 0; i < n1; ++i) {
                MapPoint *mp = lc.GetCurrentMatchedPoints()[i];
                if (mp) fin[i] = loop_index.count(mp) ? loop_index[mp] : -3;
                cur_px.push_back(cur->_features[i]->_pixel[0]); cur_px.push_back(cur->_features[i]->_pixel[1]);
            }
            for (MapPoint *mp : loop_points) for (int k = 0; k < 3; ++k) loop_pw.push_back(mp->_pos_world[k]);
            put("final", fin); put("cur_px", cur_px); put("loop_pw", loop_pw);
            vector<int32_t> f2(n2, -1);                                  // the loop keyframe's features as loop point indices (for SearchBySim3's pairs)
            for (size_t j = 0; j < n2; ++j) if (usable(loop->_features[j]->_mappoint)) f2[j] = loop_index[loop->_features[j]->_mappoint];
            put("loop_feature_point", f2);
            const vector<MapPoint *> first = lc.GetCurrentMatchedPoints();
            out[17] = lc.SearchLoopMapPoints() == (out[4] != 0) && lc.GetCurrentMatchedPoints() == first;

            // SearchFuseCandidates: the loop map points into the keyframes they came from, each with its own pose
            vector<Sim3> poses;
            for (size_t k = 0; k < group.size(); ++k) {
                poses.push_back(Sim3(group[k]->_TCW));
                Arrays f;
                f.target(group[k]);
                for (const MapPoint *mp : loop_points) f.source(mp, !usable(mp) || mp->_obs.count(group[k]->_keyframe_id) > 0);
                f.transform(without_scale(poses.back()));
                f.keep("fu" + std::to_string(k) + "_", true);
            }
            vector<vector<int>> fop;
            out[13] = matcher.SearchFuseCandidates(group, poses, loop_points, 3.0f, fop);
            vector<int32_t> r3;
            for (const auto &row : fop) for (int v : row) r3.push_back(v);
            put("fu_result", r3);
            out[14] = (double)n1; out[15] = (double)loop_points.size(); out[16] = (double)group.size();
            out[8] = map_sum(s) == m0;
        }
        for (Frame *kf : s.kfs) delete kf;
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
        for (MapPoint *mp : s.mps) delete mp;
    } catch (const std::exception &e) {
        fprintf(stderr, "widen_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // extern "C"
