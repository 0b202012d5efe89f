// ygz::LoopClosing::GlobalBundleAdjustment used the way ORB-SLAM2's LoopClosing::CorrectLoop ends, written against include/ygz only: the
// rendered loop scene of tests/cpp/fuse_surface.cpp (an "old" run of keyframes, a lead keyframe of another texture, a "revisit" run in a
// drifted world), each revisit keyframe through DetectLoop / ComputeSim3 until a loop is accepted, then SearchLoopMapPoints, CorrectLoop,
// FuseLoop and GlobalBundleAdjustment.  In this scene every map point is born with one observation, so only the fused loop map points carry
// two or more: the keyframes that observe one of those are the set the adjustment is given; the Memory form, which also takes the lead
// keyframe and the old keyframes that share nothing, has to refuse.  The program keeps the map state as bytes around each call, the problem
// the class gathered with the solver's answer, every keyframe pose and point position before and after, and the fused pairs, as named blobs
// which tests/gba_driver.py writes out for tests/test_gpu_loop_gba.py.  Built as a shared object by tests/test_gba_surface_build.py
// (-Wl,--no-undefined).
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

template <typename T> void push(vector<uint8_t> &b, const T &v) { const uint8_t *p = (const uint8_t *)&v; b.insert(b.end(), p, p + sizeof(T)); }

// poses and point positions; everything else of the map, bit for bit (pointers as ids)
void snapshot(const Scene &s, vector<uint8_t> &geometry, vector<uint8_t> &rest)
{
    geometry.clear(); rest.clear();
    for (Frame *kf : s.kfs) {
        double t[7]; kf->_TCW.to7(t);
        for (double v : t) push(geometry, v);
        push(rest, (int64_t)kf->_keyframe_id); push(rest, (int32_t)kf->_bad); push(rest, (int64_t)kf->_features.size());
        for (Feature *f : kf->_features) push(rest, (int64_t)(f->_mappoint ? (int64_t)f->_mappoint->_id : -1));
        vector<pair<unsigned long, int>> c;
        for (const auto &kv : kf->_connected_keyframe_weights) c.push_back(make_pair(kv.first->_keyframe_id, kv.second));
        std::sort(c.begin(), c.end());
        push(rest, (int64_t)c.size());
        for (const auto &kv : c) { push(rest, (int64_t)kv.first); push(rest, (int32_t)kv.second); }
        push(rest, (int64_t)kf->_cov_keyframes.size());
        for (Frame *k : kf->_cov_keyframes) push(rest, (int64_t)k->_keyframe_id);
        for (int w : kf->_cov_weights) push(rest, (int32_t)w);
    }
    for (MapPoint *mp : s.mps) {
        for (int k = 0; k < 3; ++k) push(geometry, mp->_pos_world[k]);
        push(rest, (int64_t)mp->_id); push(rest, (int32_t)mp->_bad); push(rest, (int32_t)mp->_cnt_found); push(rest, (int32_t)mp->_cnt_visible);
        push(rest, (int64_t)mp->_obs.size());
        for (const auto &ob : mp->_obs) { push(rest, (int64_t)ob.first); push(rest, ob.second ? ob.second->_pixel[0] : -1.0); push(rest, ob.second ? ob.second->_pixel[1] : -1.0); }
        const Mat &d = mp->_distinctive_desc;
        const int n = d.data ? d.rows * d.cols : 0;
        push(rest, (int32_t)n);
        for (int k = 0; k < n; ++k) rest.push_back(d.data[k]);
    }
}

}

extern "C" {

// the blob `name`: its bytes (0 when there is none)
size_t gba_blob(const char *name, const void **data)
{
    auto it = g_blobs.find(name);
    if (it == g_blobs.end()) { *data = nullptr; return 0; }
    *data = it->second.data();
    return it->second.size();
}

// The scene of fuse_run (tests/cpp/fuse_surface.cpp).  out [48]:
//   0 a loop was accepted (ComputeSim3), 1 the index of that revisit keyframe, 2 matched keyframe id, 3 current keyframe id, 4 the lead
//   keyframe's id, 5 SearchLoopMapPoints' return, 8 CorrectLoop's, 9 FuseLoop's, 10 GlobalBundleAdjustment() over every keyframe in Memory
//   (must be 0: the lead keyframe has no edge), 11 the map bit-unchanged over it, 12 GlobalBundleAdjustment(the keyframes that observe a
//   point with two observations or more), 13 everything but poses and positions bit-unchanged over it, 14 poses or positions changed,
//   15 .. 18 Stats: gba_poses, gba_points, gba_edges, gba_points_left_out, 19 .. 26 Stats::global_ba: status, lm_iterations, n_solves,
//   cg_iterations_total, cg_capped, cost_initial, cost_final, lambda, 27 keyframes given to the second call, 33 keyframes in the scene,
//   34 Stats::gba_poses of the refused call
// Blobs: the problem (ba_kf_ids [N] int64, ba_point_ids [L] int64, ba_poses / ba_poses_out [N][7], ba_fixed [N] uint8, ba_points /
//   ba_points_out [L][3], ba_edge_pose / ba_edge_point [E] int32, ba_obs [E][2], ba_K4 [4], ba_huber [1]); kf_ids [K] int64 with kf_before /
//   kf_after [K][7] every keyframe's _TCW around the second call, pt_ids [P] int64 with pt_before / pt_after [P][3] every map point's
//   _pos_world; fused [n][3] int64 (keyframe id, feature, loop point id) and fused_px [n][2] the feature's pixel, from GetFusedPairs().
// Returns 0, 1 on an exception, 2 when the vocabulary does not load.
int gba_run(int w, int h, const uint8_t *old_bgr, const float *old_depth, const double *old_T, int n_old, const uint8_t *lead_bgr,
            const float *lead_depth, const double *lead_T, const uint8_t *rev_bgr, const float *rev_depth, const double *rev_T, int n_rev,
            const double *drift, int min_kf_gap, int consistency_th, const void *vocab, size_t vocab_bytes, double *out)
{
    try {
        g_blobs.clear();
        for (int k = 0; k < 48; ++k) out[k] = 0;
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
        Frame *cur = nullptr;
        for (int k = 0; k < n_rev && !cur; ++k) {
            Frame *kf = make_keyframe(s, rev_bgr + k * fb, rev_depth + k * db, rev_T + 7 * k, D);
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
            Frame *matched = lc.GetMatchedKeyframe();
            out[2] = (double)matched->_keyframe_id; out[3] = (double)cur->_keyframe_id; out[4] = (double)lead->_keyframe_id;
            // the lead keyframe shares no map point with anyone: no covisibility
            for (Frame *r : rev) { r->_connected_keyframe_weights.erase(lead); }
            lead->_connected_keyframe_weights.clear();
            out[33] = (double)s.kfs.size();
            out[5] = lc.SearchLoopMapPoints();
            out[8] = lc.CorrectLoop(s.kfs);
            out[9] = lc.FuseLoop(s.kfs);
            vector<LoopClosing::FusedPair> fused = lc.GetFusedPairs();
            vector<int64_t> fz;
            vector<double> fpx;
            map<unsigned long, Frame *> kf_of;
            for (Frame *kf : s.kfs) kf_of[kf->_keyframe_id] = kf;
            for (const auto &fp : fused) {
                fz.push_back((int64_t)fp.keyframe_id); fz.push_back(fp.feature); fz.push_back((int64_t)fp.loop_point_id);
                const Feature *f = kf_of[fp.keyframe_id]->_features[fp.feature];
                fpx.push_back(f->_pixel[0]); fpx.push_back(f->_pixel[1]);
            }
            put("fused", fz); put("fused_px", fpx);

            vector<uint8_t> g0, r0, g1, r1, g2, r2;
            snapshot(s, g0, r0);
            out[10] = lc.GlobalBundleAdjustment();                     // every keyframe in Memory: the lead keyframe shares nothing
            out[34] = lc.GetStats().gba_poses;
            snapshot(s, g1, r1);
            out[11] = g0 == g1 && r0 == r1;

            // the keyframes that observe a point with two observations or more
            vector<Frame *> given;
            for (Frame *kf : s.kfs) {
                bool shares = false;
                for (Feature *f : kf->_features) shares |= f->_mappoint && !f->_mappoint->_bad && f->_mappoint->_obs.size() >= 2;
                if (shares) given.push_back(kf);
            }
            out[27] = (double)given.size();
            vector<int64_t> kid, pid;
            vector<double> kb, ka, pb, pa;
            for (Frame *kf : s.kfs) { kid.push_back((int64_t)kf->_keyframe_id); double t[7]; kf->_TCW.to7(t); kb.insert(kb.end(), t, t + 7); }
            for (MapPoint *mp : s.mps) { pid.push_back((int64_t)mp->_id); for (int k = 0; k < 3; ++k) pb.push_back(mp->_pos_world[k]); }
            out[12] = lc.GlobalBundleAdjustment(given);
            snapshot(s, g2, r2);
            out[13] = r1 == r2; out[14] = g1 != g2;
            for (Frame *kf : s.kfs) { double t[7]; kf->_TCW.to7(t); ka.insert(ka.end(), t, t + 7); }
            for (MapPoint *mp : s.mps) for (int k = 0; k < 3; ++k) pa.push_back(mp->_pos_world[k]);
            put("kf_ids", kid); put("kf_before", kb); put("kf_after", ka); put("pt_ids", pid); put("pt_before", pb); put("pt_after", pa);
            const LoopClosing::Stats &st = lc.GetStats();
            out[15] = st.gba_poses; out[16] = st.gba_points; out[17] = st.gba_edges; out[18] = st.gba_points_left_out;
            out[19] = st.global_ba.status; out[20] = st.global_ba.lm_iterations; out[21] = st.global_ba.n_solves;
            out[22] = st.global_ba.cg_iterations_total; out[23] = st.global_ba.cg_capped; out[24] = st.global_ba.cost_initial;
            out[25] = st.global_ba.cost_final; out[26] = st.global_ba.lambda;
            const LoopClosing::BundleProblem &bp = lc.GetBundleProblem();
            put("ba_kf_ids", vector<int64_t>(bp.keyframe_ids.begin(), bp.keyframe_ids.end()));
            put("ba_point_ids", vector<int64_t>(bp.point_ids.begin(), bp.point_ids.end()));
            put("ba_poses", bp.poses); put("ba_poses_out", bp.poses_out); put("ba_fixed", bp.fixed); put("ba_points", bp.points);
            put("ba_points_out", bp.points_out); put("ba_edge_pose", bp.edge_pose); put("ba_edge_point", bp.edge_point); put("ba_obs", bp.obs);
            put("ba_K4", vector<double>(bp.K4, bp.K4 + 4)); put("ba_huber", vector<double>(1, bp.huber_delta));
        }
        for (Frame *kf : s.kfs) delete kf;
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
        for (MapPoint *mp : s.mps) delete mp;
    } catch (const std::exception &e) {
        fprintf(stderr, "gba_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // extern "C"
