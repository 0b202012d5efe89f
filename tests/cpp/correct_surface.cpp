// ygz::LoopClosing::CorrectLoop used the way ORB-SLAM2's LoopClosing::CorrectLoop is, written against include/ygz only: the rendered loop scene
// of tests/cpp/loop_surface.cpp (an "old" run of keyframes, a lead keyframe of another texture, a "revisit" run in a drifted world), each
// revisit keyframe through DetectLoop / ComputeSim3 until a loop is accepted, then the correction.  The lead keyframe's links exist only to
// give DetectLoop its low-score neighbour: it shares no map point with any keyframe, a covisibility graph built from shared points would not
// hold them, and they are dropped before the correction.  The program keeps the map before and after, the pose graph the class gathered and
// its statistics as named blobs, which tests/correct_driver.py writes out for tests/test_gpu_loop_correct.py.
// Built as a shared object by tests/test_correct_surface_build.py (-Wl,--no-undefined).
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

map<std::string, vector<uint8_t>> g_blobs;
template <typename T> void put(const std::string &name, const vector<T> &v)
{
    vector<uint8_t> &b = g_blobs[name];
    b.resize(v.size() * sizeof(T));
    if (!v.empty()) memcpy(b.data(), v.data(), b.size());
}

// poses [K][7] by keyframe, points [P][3], then everything else a correction must not touch as one sum
void snapshot(const Scene &s, vector<double> &poses, vector<double> &points, double &rest)
{
    poses.clear(); points.clear(); rest = 0;
    for (Frame *kf : s.kfs) {
        double t[7]; kf->_TCW.to7(t);
        poses.insert(poses.end(), t, t + 7);
        rest += (double)kf->_features.size() + 3.0 * kf->_bow_vec.size() + 11.0 * kf->_cov_keyframes.size() + (kf->_bad ? 1 : 0);
        for (const auto &c : kf->_connected_keyframe_weights) rest += c.second + 0.001 * c.first->_keyframe_id;
        for (Feature *f : kf->_features) rest += f->_pixel[0] + (f->_mappoint ? 1.0 + 1e-3 * (double)f->_mappoint->_id : 0.0) + f->_level;
    }
    for (MapPoint *mp : s.mps) {
        for (int k = 0; k < 3; ++k) points.push_back(mp->_pos_world[k]);
        rest += (double)mp->_obs.size() + mp->_bad + mp->_cnt_found + mp->_cnt_visible;
    }
}
}

extern "C" {

// the blob `name`: its bytes (0 when there is none)
size_t correct_blob(const char *name, const void **data)
{
    auto it = g_blobs.find(name);
    if (it == g_blobs.end()) { *data = nullptr; return 0; }
    *data = it->second.data();
    return it->second.size();
}

// The scene of loop_run (tests/cpp/loop_surface.cpp) without the other texture's run.  out [32]:
//   0 a loop was accepted (ComputeSim3), 1 the index of that revisit keyframe, 2 matched keyframe id, 3 current keyframe id,
//   4 CorrectLoop(keyframes)'s return, 5 a second CorrectLoop() (the Memory form), 6 the map bit-unchanged over the second call,
//   7 everything but poses and point positions unchanged over the first, 8 the lead keyframe's id, 9 .. 13 Stats: vertices, tree edges,
//   covisibility edges, loop edges, points moved, 14 keyframes left out, 15 .. 19 status, lm_iterations, n_solves, cg_iterations_total,
//   cg_capped, 20 .. 22 cost_initial, cost_final, lambda, 23 CorrectLoop before any accepted loop (must be 0)
// Blobs: K4; kf_ids [K]; poses_before / poses_after [K][7]; pt_before / pt_after [P][3]; pt_kf [P] the keyframe id that observes the point;
//   pt_px [P][2] its pixel there; left_out; the pose graph: g_ids, g_S, g_S_out, g_fixed, g_edges, g_M; S_cw [8].
// Returns 0, 1 on an exception, 2 when the vocabulary does not load.
int correct_run(int w, int h, const uint8_t *old_bgr, const float *old_depth, const double *old_T, int n_old, const uint8_t *lead_bgr,
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
        Frame *lead = make_keyframe(s, lead_bgr, lead_depth, lead_T, D);
        rev.push_back(lead);
        LoopClosing lc;
        lc._option._min_kf_gap = min_kf_gap; lc._option._consistency_th = consistency_th;
        out[23] = lc.CorrectLoop(s.kfs);
        Frame *cur = nullptr;
        for (int k = 0; k < n_rev && !cur; ++k) {
            Frame *kf = make_keyframe(s, rev_bgr + k * fb, rev_depth + k * db, rev_T + 7 * k, D);
            // neighbours in the run: 120 with the one before, 100 with the one before that (an edge of the essential graph), 50 further back
            for (size_t r = 0; r < rev.size(); ++r) {
                const size_t gap = rev.size() - r;
                link_keyframes(kf, rev[r], rev[r] == lead ? 50 : (gap == 1 ? 120 : (gap == 2 ? 100 : 50)));
            }
            rev.push_back(kf);
            for (Frame *r : rev) { r->_cov_keyframes.clear(); r->_cov_weights.clear(); r->UpdateBestCovisibles(); }
            if (lc.DetectLoop(kf, s.kfs) && lc.ComputeSim3()) { cur = kf; out[1] = k; }
        }
        if (cur) {
            out[0] = 1;
            out[2] = (double)lc.GetMatchedKeyframe()->_keyframe_id; out[3] = (double)cur->_keyframe_id; out[8] = (double)lead->_keyframe_id;
            // the lead keyframe shares no map point with anyone: no covisibility
            for (Frame *r : rev) { r->_connected_keyframe_weights.erase(lead); }
            lead->_connected_keyframe_weights.clear();
            const Matrix3d K = cam.GetCameraMatrix();
            put("K4", vector<double>{ K(0, 0), K(1, 1), K(0, 2), K(1, 2) });
            vector<double> S8(8);
            lc.GetCorrectedPose().to8(S8.data());
            put("S_cw", S8);
            vector<int32_t> ids, pt_kf;
            vector<double> pt_px;
            for (Frame *kf : s.kfs) ids.push_back((int32_t)kf->_keyframe_id);
            for (MapPoint *mp : s.mps) {
                const auto &ob = *mp->_obs.begin();
                pt_kf.push_back((int32_t)ob.first);
                pt_px.push_back(ob.second->_pixel[0]); pt_px.push_back(ob.second->_pixel[1]);
            }
            put("kf_ids", ids); put("pt_kf", pt_kf); put("pt_px", pt_px);
            vector<double> p0, x0, p1, x1, p2, x2;
            double r0, r1, r2;
            snapshot(s, p0, x0, r0);
            out[4] = lc.CorrectLoop(s.kfs);
            snapshot(s, p1, x1, r1);
            out[7] = r0 == r1;
            const LoopClosing::Stats st = lc.GetStats();
            const LoopClosing::PoseGraph g = lc.GetPoseGraph();
            out[5] = lc.CorrectLoop();
            snapshot(s, p2, x2, r2);
            out[6] = p1.size() == p2.size() && x1.size() == x2.size() && memcmp(p1.data(), p2.data(), p1.size() * 8) == 0
                     && memcmp(x1.data(), x2.data(), x1.size() * 8) == 0 && r1 == r2;
            put("poses_before", p0); put("poses_after", p1); put("pt_before", x0); put("pt_after", x1);
            out[9] = st.correct_vertices; out[10] = st.correct_tree_edges; out[11] = st.correct_covisibility_edges; out[12] = st.correct_loop_edges;
            out[13] = st.correct_points_moved; out[14] = (double)st.correct_left_out.size();
            out[15] = st.pose_graph.status; out[16] = st.pose_graph.lm_iterations; out[17] = st.pose_graph.n_solves;
            out[18] = st.pose_graph.cg_iterations_total; out[19] = st.pose_graph.cg_capped;
            out[20] = st.pose_graph.cost_initial; out[21] = st.pose_graph.cost_final; out[22] = st.pose_graph.lambda;
            vector<int32_t> lo, gid;
            for (unsigned long id : st.correct_left_out) lo.push_back((int32_t)id);
            for (unsigned long id : g.keyframe_ids) gid.push_back((int32_t)id);
            put("left_out", lo); put("g_ids", gid); put("g_S", g.S); put("g_S_out", g.S_out); put("g_fixed", g.fixed); put("g_edges", g.edges);
            put("g_M", g.M);
        }
        for (Frame *kf : s.kfs) delete kf;
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
        for (MapPoint *mp : s.mps) delete mp;
    } catch (const std::exception &e) {
        fprintf(stderr, "correct_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // extern "C"
