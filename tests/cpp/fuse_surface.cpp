// ygz::LoopClosing::FuseLoop / UpdateCovisibility / ReplaceMapPoint and Matcher::ComputeDistinctiveDescriptors used the way ORB-SLAM2's
// LoopClosing::CorrectLoop goes on after its pose graph, written against include/ygz only: the rendered loop scene of
// tests/cpp/correct_surface.cpp (an "old" run of keyframes, a lead keyframe of another texture, a "revisit" run in a drifted world), each
// revisit keyframe through DetectLoop / ComputeSim3 until a loop is accepted, then SearchLoopMapPoints, CorrectLoop and FuseLoop.  The program
// keeps the whole map state as bytes before and after each call, the fused pairs with what a check of their placement needs, the descriptors
// it gathered for every loop map point that gained an observation, and every keyframe's covisibility from UpdateCovisibility(all, all) beside
// Frame::UpdateConnections() on the same state, as named blobs which tests/fuse_driver.py writes out for tests/test_gpu_loop_fuse.py.
// Built as a shared object by tests/test_fuse_surface_build.py (-Wl,--no-undefined).
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

int good_points(const Scene &s) { int n = 0; for (MapPoint *mp : s.mps) n += !mp->_bad; return n; }

// per keyframe: id, n, (id, weight) x n of _connected_keyframe_weights by id, m, (id, weight) x m of _cov_keyframes / _cov_weights in their order
void covisibility_record(const Frame *kf, vector<int32_t> &out)
{
    out.push_back((int32_t)kf->_keyframe_id);
    vector<pair<unsigned long, int>> c;
    for (const auto &kv : kf->_connected_keyframe_weights) c.push_back(make_pair(kv.first->_keyframe_id, kv.second));
    std::sort(c.begin(), c.end());
    out.push_back((int32_t)c.size());
    for (const auto &kv : c) { out.push_back((int32_t)kv.first); out.push_back(kv.second); }
    out.push_back((int32_t)kf->_cov_keyframes.size());
    for (size_t i = 0; i < kf->_cov_keyframes.size(); ++i) { out.push_back((int32_t)kf->_cov_keyframes[i]->_keyframe_id); out.push_back(kf->_cov_weights[i]); }
}

struct Covis { map<Frame *, int> connected; vector<Frame *> kfs; vector<int> weights; };
void save(const Scene &s, vector<Covis> &c)
{
    c.clear();
    for (Frame *kf : s.kfs) c.push_back(Covis{ kf->_connected_keyframe_weights, kf->_cov_keyframes, kf->_cov_weights });
}
void restore(const Scene &s, const vector<Covis> &c)
{
    for (size_t i = 0; i < s.kfs.size(); ++i) {
        s.kfs[i]->_connected_keyframe_weights = c[i].connected; s.kfs[i]->_cov_keyframes = c[i].kfs; s.kfs[i]->_cov_weights = c[i].weights;
    }
}

int weight_to(const Frame *a, Frame *b)
{
    auto it = a->_connected_keyframe_weights.find(b);
    return it == a->_connected_keyframe_weights.end() ? 0 : it->second;
}
}

extern "C" {

// the blob `name`: its bytes (0 when there is none)
size_t fuse_blob(const char *name, const void **data)
{
    auto it = g_blobs.find(name);
    if (it == g_blobs.end()) { *data = nullptr; return 0; }
    *data = it->second.data();
    return it->second.size();
}

// The scene of correct_run (tests/cpp/correct_surface.cpp).  out [48]:
//   0 a loop was accepted (ComputeSim3), 1 the index of that revisit keyframe, 2 matched keyframe id, 3 current keyframe id, 4 the lead
//   keyframe's id, 5 SearchLoopMapPoints' return, 6 FuseLoop before CorrectLoop (must be 0), 7 the map bit-unchanged over it, 8 CorrectLoop's
//   return, 9 the first FuseLoop(keyframes), 10 poses and point positions bit-unchanged over it, 11 a second FuseLoop() (the Memory form),
//   12 the map bit-unchanged over the second, 13 / 14 good map points before / after, 15 .. 23 Stats: fuse_current_replaced,
//   fuse_current_added, fuse_targets, fuse_hits, fuse_replaced, fuse_added, fuse_conflicts, fuse_descriptors, fuse_rows, 24 / 25 the current
//   keyframe's weight to the matched keyframe before / after, 26 that weight summed over the matched keyframe and its connected keyframes
//   after, 27 GetMatches().size(), 28 total_matches, 29 features of the current keyframe with a good loop map point before the call,
//   30 features that point to a bad map point after, 31 features / observations that break f->_mappoint == p <=> p->_obs[id(f)] == f after,
//   32 UpdateCovisibility(all, all)'s return, 33 keyframes, 34 the map changed over the first FuseLoop (it must), 35 the loop map points
// Blobs: K4; kf_ids [K]; fused [n][4] int64 (keyframe id, feature, loop point id, replaced point id or -1); fused_px [n][2] the feature's
//   pixel; fused_pw [n][3] the loop point; fused_pred [n] its predicted level in that keyframe (Matcher::PointAttributes' dmax over the
//   distance, by comparisons); dd_offsets [G + 1], dd_desc [.][32] the observations' descriptors of every loop map point that gained an
//   observation (in _obs key order), dd_got [G][32] its _distinctive_desc; cov_dev / cov_host: per keyframe its covisibility record after
//   UpdateCovisibility(all, all) and after Frame::UpdateConnections() on the same state; cov_before: that state.
// Returns 0, 1 on an exception, 2 when the vocabulary does not load.
int fuse_run(int w, int h, const uint8_t *old_bgr, const float *old_depth, const double *old_T, int n_old, const uint8_t *lead_bgr,
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
            const Matrix3d K = cam.GetCameraMatrix();
            put("K4", vector<double>{ K(0, 0), K(1, 1), K(0, 2), K(1, 2) });
            vector<int32_t> ids;
            for (Frame *kf : s.kfs) ids.push_back((int32_t)kf->_keyframe_id);
            put("kf_ids", ids);
            out[33] = (double)s.kfs.size();

            out[5] = lc.SearchLoopMapPoints();
            out[27] = (double)lc.GetMatches().size(); out[28] = lc.GetStats().total_matches; out[35] = (double)lc.GetLoopMapPoints().size();
            vector<uint8_t> g0, r0, g1, r1, g2, r2, g3, r3;
            snapshot(s, g0, r0);
            out[6] = lc.FuseLoop(s.kfs);
            snapshot(s, g1, r1);
            out[7] = g0 == g1 && r0 == r1;
            out[8] = lc.CorrectLoop(s.kfs);
            snapshot(s, g1, r1);
            for (MapPoint *mp : lc.GetCurrentMatchedPoints()) out[29] += mp && !mp->_bad;
            out[13] = good_points(s);
            out[24] = weight_to(cur, matched);
            out[9] = lc.FuseLoop(s.kfs);
            snapshot(s, g2, r2);
            out[10] = g1 == g2; out[34] = r1 != r2;
            out[14] = good_points(s);
            const LoopClosing::Stats st = lc.GetStats();
            const vector<LoopClosing::FusedPair> fused = lc.GetFusedPairs();
            out[11] = lc.FuseLoop();
            snapshot(s, g3, r3);
            out[12] = g2 == g3 && r2 == r3;
            out[15] = st.fuse_current_replaced; out[16] = st.fuse_current_added; out[17] = st.fuse_targets; out[18] = st.fuse_hits;
            out[19] = st.fuse_replaced; out[20] = st.fuse_added; out[21] = st.fuse_conflicts; out[22] = st.fuse_descriptors; out[23] = st.fuse_rows;
            out[25] = weight_to(cur, matched);
            out[26] = weight_to(cur, matched);
            for (const auto &c : matched->_connected_keyframe_weights) if (c.first != matched && c.first != cur) out[26] += weight_to(cur, c.first);

            // the invariants over all keyframes and points
            for (Frame *kf : s.kfs)
                for (Feature *f : kf->_features) {
                    MapPoint *p = f->_mappoint;
                    if (!p) continue;
                    if (p->_bad) out[30] += 1;
                    auto it = p->_obs.find(kf->_keyframe_id);
                    if (it == p->_obs.end() || it->second != f) out[31] += 1;
                }
            for (MapPoint *p : s.mps)
                for (const auto &ob : p->_obs)
                    if (!ob.second || ob.second->_mappoint != p || !ob.second->_frame || ob.second->_frame->_keyframe_id != ob.first) out[31] += 1;

            // the fused pairs with what their placement check needs
            map<unsigned long, Frame *> kf_of;
            for (Frame *kf : s.kfs) kf_of[kf->_keyframe_id] = kf;
            map<unsigned long, MapPoint *> mp_of;
            for (MapPoint *mp : s.mps) mp_of[mp->_id] = mp;
            vector<int64_t> fz;
            vector<double> fpx, fpw;
            vector<int32_t> fpred;
            const int levels = cur->_option._pyramid_level;
            for (const auto &fp : fused) {
                fz.push_back((int64_t)fp.keyframe_id); fz.push_back(fp.feature); fz.push_back((int64_t)fp.loop_point_id); fz.push_back(fp.replaced_point_id);
                Frame *kf = kf_of[fp.keyframe_id];
                MapPoint *L = mp_of[fp.loop_point_id];
                const Feature *f = kf->_features[fp.feature];
                fpx.push_back(f->_pixel[0]); fpx.push_back(f->_pixel[1]);
                for (int k = 0; k < 3; ++k) fpw.push_back(L->_pos_world[k]);
                Matcher::PointAttr a;
                int pred = -1;
                if (Matcher::PointAttributes(L, a)) {
                    const double ratio = a.dmax / (kf->_TCW * L->_pos_world).norm();
                    pred = levels - 1;
                    for (int n = levels - 2; n >= 0; --n) if (ratio <= (double)(1 << n)) pred = n;
                }
                fpred.push_back(pred);
            }
            put("fused", fz); put("fused_px", fpx); put("fused_pw", fpw); put("fused_pred", fpred);

            // every loop map point that gained an observation: its observations' descriptors in key order, and what the class stored
            std::set<unsigned long> gained_ids;
            for (const auto &fp : fused) gained_ids.insert(fp.loop_point_id);
            vector<int32_t> dd_off(1, 0);
            vector<uint8_t> dd_desc, dd_got;
            for (MapPoint *L : lc.GetLoopMapPoints()) {
                if (!gained_ids.count(L->_id)) continue;
                for (const auto &ob : L->_obs) if (ob.second) dd_desc.insert(dd_desc.end(), ob.second->_desc.data, ob.second->_desc.data + 32);
                dd_off.push_back((int32_t)(dd_desc.size() / 32));
                const Mat &d = L->_distinctive_desc;
                for (int k = 0; k < 32; ++k) dd_got.push_back(d.data && d.rows * d.cols == 32 ? d.data[k] : 0);
            }
            put("dd_offsets", dd_off); put("dd_desc", dd_desc); put("dd_got", dd_got);

            // UpdateCovisibility(all, all) beside Frame::UpdateConnections() per keyframe, each on the state FuseLoop left
            vector<Covis> state;
            save(s, state);
            vector<int32_t> host, dev, before;
            for (Frame *kf : s.kfs) covisibility_record(kf, before);
            for (Frame *kf : s.kfs) {
                restore(s, state);
                kf->UpdateConnections();
                covisibility_record(kf, host);
            }
            restore(s, state);
            out[32] = lc.UpdateCovisibility(s.kfs, s.kfs);
            for (Frame *kf : s.kfs) covisibility_record(kf, dev);
            put("cov_host", host); put("cov_dev", dev); put("cov_before", before);
        }
        for (Frame *kf : s.kfs) delete kf;
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
        for (MapPoint *mp : s.mps) delete mp;
    } catch (const std::exception &e) {
        fprintf(stderr, "fuse_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // extern "C"
