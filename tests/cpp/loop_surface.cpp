// ygz::LoopClosing used the way LocalMapping.cpp:330 would use it, written against include/ygz only: an "old" run of
// keyframes with map points from their depth images and a covisibility graph, then a "revisit" run over the same region expressed in a
// drifted world (a Sim3 D: poses (R R_d^T, s_d t - R R_d^T t_d), map points D(X)), connected among themselves only, each keyframe handed to
// DetectLoop and, when it fires, ComputeSim3; then a run of another texture.  Also the Sim3 algebra on plain arrays.
// Built as a shared object by tests/test_loop_surface_build.py (-Wl,--no-undefined) and called through ctypes by tests/loop_driver.py.
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <chrono>
#include <cstdio>
#include <cstring>
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
        for (Feature *f : kf->_features) sum += f->_pixel[0] + (f->_mappoint ? 1.0 : 0.0);
    }
    for (MapPoint *mp : s.mps) sum += mp->_pos_world[0] + mp->_pos_world[1] + mp->_pos_world[2] + mp->_obs.size() + mp->_bad + mp->_cnt_found;
    return sum;
}
}

extern "C" {

// Sim3 algebra: a, b as qx qy qz qw tx ty tz s; out [8] a * b, out [8 .. 15] a^-1, out [16 .. 18] a * p, out [19 .. 26] a * SE3(b's first 7)
void loop_sim3_algebra(const double *a, const double *b, const double *p, double *out)
{
    const Sim3 A = Sim3::from8(a), B = Sim3::from8(b);
    (A * B).to8(out);
    A.inverse().to8(out + 8);
    const Vector3d q = A * Vector3d(p[0], p[1], p[2]);
    for (int k = 0; k < 3; ++k) out[16 + k] = q[k];
    (A * SE3::from7(b)).to8(out + 19);
}

// old: n_old keyframes bgr [n][h][w][3], depth [n][h][w], true T_cw [n][7] (the map's world); lead: one keyframe of another texture that
// starts the revisit run; rev: n_rev keyframes of the revisit run (true poses); drift [8]: D as qx qy qz qw tx ty tz s; oth: n_oth keyframes
// of another texture.  min_kf_gap, consistency_th: the options.  Per call (revisit keyframes, then the other texture's), out [q][40]:
//   0 DetectLoop, 1 ComputeSim3 (0 when not called), 2 matched keyframe id (-1), 3..10 S12, 11..18 corrected pose S_cw, 19 GetMatches size,
//   20 map checksum unchanged over both calls, 21 Memory form equal (detect, matched, S12 bits), 22 candidates, 23 a candidate connected
//   to the keyframe, 24 largest consistency, 25 refined inliers of the match, 26 its BoW pairs, 27 ms DetectLoop, 28 ms ComputeSim3,
//   29 keyframe id, 30 minScore, 31 RANSAC inliers of the match, 32 enough-consistent candidates, 33 the keyframe's words, 34 the fewest
//   words of a connected keyframe, 35 the best BoW score of a keyframe not connected to it, 36 the keyframe's connections
// Returns 0, 1 on an exception, 2 when the vocabulary does not load.
int loop_run(int w, int h, const uint8_t *old_bgr, const float *old_depth, const double *old_T, int n_old, const uint8_t *lead_bgr,
             const float *lead_depth, const double *lead_T, const uint8_t *rev_bgr, const float *rev_depth, const double *rev_T, int n_rev,
             const double *drift, const uint8_t *oth_bgr, const float *oth_depth, const double *oth_T, int n_oth, int min_kf_gap,
             int consistency_th, const void *vocab, size_t vocab_bytes, double *out)
{
    try {
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
        // the old run: covisibility with the two neighbours on each side
        vector<Frame *> old;
        for (int k = 0; k < n_old; ++k) old.push_back(make_keyframe(s, old_bgr + k * fb, old_depth + k * db, old_T + 7 * k, I));
        for (int i = 0; i < n_old; ++i)
            for (int j = i + 1; j < n_old && j <= i + 2; ++j) link_keyframes(old[i], old[j], 100 - 20 * (j - i));
        for (Frame *kf : old) kf->UpdateBestCovisibles();
        // the revisit run: a keyframe of another texture first (its neighbour of low BoW score), then the keyframes over the old region
        vector<Frame *> rev;
        rev.push_back(make_keyframe(s, lead_bgr, lead_depth, lead_T, D));
        LoopClosing lc, lc_mem;
        for (LoopClosing *l : { &lc, &lc_mem }) { l->_option._min_kf_gap = min_kf_gap; l->_option._consistency_th = consistency_th; }
        auto one_call = [&](LoopClosing &L, LoopClosing &Lm, Frame *kf, double *o) {
            for (int k = 0; k < 40; ++k) o[k] = 0;
            const double m0 = map_sum(s);
            const vector<Frame *> all = s.kfs;
            auto t0 = std::chrono::steady_clock::now();
            const bool det = L.DetectLoop(kf, all);
            o[27] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            bool ok = false;
            if (det) {
                t0 = std::chrono::steady_clock::now();
                ok = L.ComputeSim3();
                o[28] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            }
            o[0] = det; o[1] = ok;
            o[2] = L.GetMatchedKeyframe() ? (double)L.GetMatchedKeyframe()->_keyframe_id : -1.0;
            L.GetSim3().to8(o + 3);
            L.GetCorrectedPose().to8(o + 11);
            o[19] = (double)L.GetMatches().size();
            const LoopClosing::Stats &st = L.GetStats();
            o[22] = (double)st.candidates.size();
            for (unsigned long id : st.candidates) {
                Frame *c = Memory::GetKeyFrame(id);
                if (c == kf || kf->_connected_keyframe_weights.count(c)) o[23] = 1;
            }
            for (int c : st.consistency) o[24] = std::max(o[24], (double)c);
            for (size_t c = 0; c < st.consistent.size(); ++c)
                if (L.GetMatchedKeyframe() && st.consistent[c] == L.GetMatchedKeyframe()->_keyframe_id && c < st.refined_inliers.size()) {
                    o[25] = st.refined_inliers[c]; o[26] = st.bow_pairs[c]; o[31] = st.ransac_inliers[c];
                }
            o[29] = (double)kf->_keyframe_id;
            o[30] = st.min_score;
            o[32] = (double)st.consistent.size();
            // the BoW picture: the keyframe's words, the fewest words of a connected keyframe, the best score of one not connected
            o[33] = (double)kf->_bow_vec.size();
            o[36] = (double)kf->_connected_keyframe_weights.size();
            o[34] = 1e9;
            for (const auto &c : kf->_connected_keyframe_weights) o[34] = std::min(o[34], (double)c.first->_bow_vec.size());
            for (Frame *k : all)
                if (k != kf && !kf->_connected_keyframe_weights.count(k)) o[35] = std::max(o[35], Frame::_vocab->score(kf->_bow_vec, k->_bow_vec));
            // the Memory form, in lockstep
            const bool det2 = Lm.DetectLoop(kf);
            const bool ok2 = det2 && Lm.ComputeSim3();
            double a[8], b[8];
            L.GetSim3().to8(a); Lm.GetSim3().to8(b);
            o[21] = det2 == det && ok2 == ok && Lm.GetMatchedKeyframe() == L.GetMatchedKeyframe() && memcmp(a, b, sizeof a) == 0
                    && Lm.GetMatches() == L.GetMatches();
            o[20] = map_sum(s) == m0;
        };
        int q = 0;
        for (int k = 0; k < n_rev; ++k, ++q) {
            Frame *kf = make_keyframe(s, rev_bgr + k * fb, rev_depth + k * db, rev_T + 7 * k, D);
            for (Frame *r : rev) link_keyframes(kf, r, 50);
            rev.push_back(kf);
            for (Frame *r : rev) { r->_cov_keyframes.clear(); r->_cov_weights.clear(); r->UpdateBestCovisibles(); }
            one_call(lc, lc_mem, kf, out + 40 * (size_t)q);
        }
        // another texture: its own keyframes, connected among themselves, against the whole map
        LoopClosing lo, lo_mem;
        for (LoopClosing *l : { &lo, &lo_mem }) { l->_option._min_kf_gap = min_kf_gap; l->_option._consistency_th = consistency_th; }
        vector<Frame *> oth;
        for (int k = 0; k < n_oth; ++k, ++q) {
            Frame *kf = make_keyframe(s, oth_bgr + k * fb, oth_depth + k * db, oth_T + 7 * k, I);
            for (Frame *r : oth) link_keyframes(kf, r, 50);
            oth.push_back(kf);
            one_call(lo, lo_mem, kf, out + 40 * (size_t)q);
        }
        for (Frame *kf : s.kfs) delete kf;
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
        for (MapPoint *mp : s.mps) delete mp;
    } catch (const std::exception &e) {
        fprintf(stderr, "loop_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // extern "C"
