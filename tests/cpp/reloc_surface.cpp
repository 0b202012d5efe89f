// ygz::Relocalizer used the way the stub at src/Module/VisualOdometry.cpp:101-104 would use it, written against include/ygz
// only: a map of keyframes built through the class surfaces (InitFrame, FeatureDetector, Memory, ComputeBoW; map points from the keyframes'
// depth images, as tests/cpp/bench_surface.cpp makes them), then kidnapped frames relocalised with Relocalize, and a relocalised frame tracked
// into the next one (SparseImageAlignment, BruteForceMatch, OptimizeCurrentPoseOnly).  Also Vocabulary::score on hand-built vectors.
// Built as a shared object by tests/test_reloc_surface_build.py (-Wl,--no-undefined) and called through ctypes by tests/test_gpu_relocalize.py.
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <cstdio>
#include <cstring>
#include <chrono>
using namespace ygz;

extern "C" {

// Vocabulary::score of two BowVectors given as (word id, value) arrays; blob: a vocabulary file (scoring type in its header)
double reloc_score(const void *blob, size_t bytes, const uint32_t *w1, const double *v1, int n1, const uint32_t *w2, const double *v2, int n2)
{
    DBoW3::Vocabulary voc;
    if (blob) voc.loadFromMemory(blob, bytes);
    DBoW3::BowVector a, b;
    for (int i = 0; i < n1; ++i) a[w1[i]] = v1[i];
    for (int i = 0; i < n2; ++i) b[w2[i]] = v2[i];
    return voc.score(a, b);
}

// keyframes: bgr [n_kf][h][w][3], depth [n_kf][h][w] (metres), T_kf [n_kf][7]; queries bgr [n_q][h][w][3]; next [n_q][h][w][3] (the frame after
// each query, may be NULL).  Per query q, out [q][40]:
//   0 ok, 1..7 T_cw after Relocalize (from identity), 8..11 stats (candidates, pnp_problems, ransac_inliers, final_inliers), 12 features,
//   13 matched keyframe id (-1), 14 Memory form equal (ok, T bit for bit, features, matched), 15 features / _bow_vec / _feature_vec empty
//   after a failure and _TCW bits unchanged (1 when ok), 16 map unchanged by a failed call (1 when ok), 17 relocalised inlier features matched in
//   the next frame (BruteForceMatch, gated by the aligned projection), 18 next frame inliers after OptimizeCurrentPoseOnly, 19..25 T_cw of the next frame after it,
//   26 ms of the Relocalize call (host clock), 27..33 T_cw of the next frame after SparseImageAlignment
// Returns 0, 1 on an exception, 2 when the vocabulary does not load.
int reloc_run(int w, int h, const uint8_t *kf_bgr, const float *kf_depth, const double *T_kf, int n_kf, const uint8_t *q_bgr, int n_q,
              const uint8_t *next_bgr, const void *vocab, size_t vocab_bytes, double *out)
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
        vector<Frame *> kfs;
        vector<MapPoint *> mps;
        const size_t fb = (size_t)w * h * 3;
        for (int k = 0; k < n_kf; ++k) {
            Frame *kf = new Frame;
            kf->_id = (unsigned long)k;
            kf->_color = cv::Mat(h, w, CV_8UC3, const_cast<uint8_t *>(kf_bgr + (size_t)k * fb));
            kf->InitFrame();
            kf->_TCW = SE3::from7(T_kf + 7 * k);
            detector.Detect(kf);
            detector.ComputeAngleAndDescriptor(kf);
            Memory::RegisterKeyFrame(kf);
            const float *D = kf_depth + (size_t)k * w * h;
            for (Feature *f : kf->_features) {
                const double d = D[(size_t)(int)f->_pixel[1] * w + (int)f->_pixel[0]];
                if (!(d > 0)) continue;
                MapPoint *mp = Memory::CreateMapPoint();
                mp->_pos_world = cam.Pixel2World(f->_pixel, kf->_TCW, d);
                mp->_obs[kf->_keyframe_id] = f;
                f->_mappoint = mp; f->_depth = d;
                mps.push_back(mp);
            }
            kf->ComputeBoW();
            kfs.push_back(kf);
        }
        auto map_sum = [&]() {
            double s = 0;
            for (Frame *kf : kfs) { double t[7]; kf->_TCW.to7(t); for (double v : t) s += v; s += (double)kf->_features.size() + kf->_bow_vec.size(); }
            for (MapPoint *mp : mps) s += mp->_pos_world[0] + mp->_pos_world[1] + mp->_pos_world[2] + mp->_cnt_found + mp->_cnt_visible + mp->_obs.size() + mp->_bad;
            return s;
        };
        for (int q = 0; q < n_q; ++q) {
            double *o = out + 40 * (size_t)q;
            for (int k = 0; k < 40; ++k) o[k] = 0;
            Frame *cur = new Frame;
            cur->_id = 1000 + (unsigned long)q;
            cur->_color = cv::Mat(h, w, CV_8UC3, const_cast<uint8_t *>(q_bgr + (size_t)q * fb));
            cur->InitFrame();
            cur->_TCW = SE3();                                       // kidnapped: the pose is lost
            double T0[7]; cur->_TCW.to7(T0);
            const double m0 = map_sum();
            Relocalizer reloc;
            const auto t0 = std::chrono::steady_clock::now();
            const bool ok = reloc.Relocalize(cur, kfs);
            o[26] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            double T[7]; cur->_TCW.to7(T);
            o[0] = ok;
            for (int k = 0; k < 7; ++k) o[1 + k] = T[k];
            const Relocalizer::Stats &st = reloc.GetStats();
            o[8] = st.candidates; o[9] = st.pnp_problems; o[10] = st.ransac_inliers; o[11] = st.final_inliers;
            o[12] = (double)cur->_features.size();
            o[13] = reloc.GetMatchedKeyframe() ? (double)reloc.GetMatchedKeyframe()->_keyframe_id : -1.0;
            // the Memory form on a fresh frame of the same image
            {
                Frame *c2 = new Frame;
                c2->_color = cur->_color;
                c2->InitFrame();
                Relocalizer r2;
                const bool ok2 = r2.Relocalize(c2);
                double T2[7]; c2->_TCW.to7(T2);
                o[14] = ok2 == ok && memcmp(T, T2, sizeof T) == 0 && c2->_features.size() == cur->_features.size()
                        && r2.GetMatchedKeyframe() == reloc.GetMatchedKeyframe();
                delete c2;
            }
            o[15] = ok ? 1 : (cur->_features.empty() && cur->_bow_vec.empty() && cur->_feature_vec.empty() && memcmp(T, T0, sizeof T) == 0);
            o[16] = ok ? 1 : map_sum() == m0;
            if (ok && next_bgr) {
                // VO_GOOD on the next frame with the relocalised frame as the reference: TrackRefFrame (SparseImageAlignment), then the
                // relocalised features matched into the next frame's own (Detect, BruteForceMatch with cross-check, kept within 5 px of the
                // aligned projection) and OptimizeCurrentPoseOnly over those matches
                Frame *nx = new Frame;
                nx->_color = cv::Mat(h, w, CV_8UC3, const_cast<uint8_t *>(next_bgr + (size_t)q * fb));
                nx->InitFrame();
                nx->_TCW = cur->_TCW;
                Matcher matcher;
                matcher.SparseImageAlignment(cur, nx);
                double Ta[7]; nx->_TCW.to7(Ta);
                for (int k = 0; k < 7; ++k) o[27 + k] = Ta[k];
                detector.Detect(nx);
                detector.ComputeAngleAndDescriptor(nx);
                vector<DMatch> dm;
                matcher.BruteForceMatch(cur, nx, dm, true);
                vector<Feature *> keep;
                vector<char> kept(nx->_features.size(), 0);
                for (const DMatch &m : dm) {
                    Feature *rf = cur->_features[m.queryIdx];
                    if (rf->_bad || !rf->_mappoint) continue;
                    // the gate of a guided search: within 5 px of where the aligned pose projects the map point
                    const Vector2d pp = cam.World2Pixel(rf->_mappoint->_pos_world, nx->_TCW);
                    const Vector2d &pn = nx->_features[m.trainIdx]->_pixel;
                    if ((pp[0] - pn[0]) * (pp[0] - pn[0]) + (pp[1] - pn[1]) * (pp[1] - pn[1]) > 25.0) continue;
                    nx->_features[m.trainIdx]->_mappoint = rf->_mappoint;
                    keep.push_back(nx->_features[m.trainIdx]);
                    kept[m.trainIdx] = 1;
                }
                for (size_t k = 0; k < nx->_features.size(); ++k) if (!kept[k]) delete nx->_features[k];
                nx->_features = keep;
                o[17] = (double)keep.size();
                if (!nx->_features.empty()) ba::OptimizeCurrentPoseOnly(nx);
                int inl = 0;
                for (Feature *f : nx->_features) inl += !f->_bad;
                o[18] = inl;
                double Tn[7]; nx->_TCW.to7(Tn);
                for (int k = 0; k < 7; ++k) o[19 + k] = Tn[k];
                delete nx;
            }
            delete cur;
        }
        for (Frame *kf : kfs) delete kf;
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
        for (MapPoint *mp : mps) delete mp;
    } catch (const std::exception &e) {
        fprintf(stderr, "reloc_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // extern "C"
