// ygz::KeyFrameDatabase used the way INTEGRATION.md shows, written against include/ygz only, on the scenes of tests/cpp/loop_surface.cpp and
// tests/cpp/reloc_surface.cpp (the arrays come from tests/loop_driver.py and tests/reloc_driver.py): the loop-closing run and the
// relocalisation run, each with no database (mode 0), with a database that holds every keyframe (mode 1) and with one that holds every second
// keyframe (mode 2).  Every outcome is written out so that the caller can compare the three bit for bit; in modes 1 and 2 every Query is
// compared here with common words counted and Frame::_vocab->score called per keyframe, and the return values of Add / Erase are checked.
// Also the host loop the database replaces, timed on BoW vectors given as arrays (tools/kfdb_bench.py).
// Built as a shared object by tests/test_kfdb_surface_build.py (-Wl,--no-undefined) and called through ctypes by tests/kfdb_driver.py.
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

int common_words(const DBoW3::BowVector &a, const DBoW3::BowVector &b)
{
    int n = 0;
    auto i = a.begin(), j = b.begin();
    while (i != a.end() && j != b.end()) {
        if (i->first == j->first) { ++n; ++i; ++j; }
        else if (i->first < j->first) ++i;
        else ++j;
    }
    return n;
}

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// the hits of v against what the host functions give for every keyframe the database holds: the same set, by keyframe id, the same bits
bool query_equals_host(KeyFrameDatabase &db, const DBoW3::BowVector &v, const vector<Frame *> &kfs, const vector<KeyFrameDatabase::Hit> &hits)
{
    vector<KeyFrameDatabase::Hit> want;
    for (Frame *k : kfs) {
        if (!db.Has(k)) continue;
        const int c = common_words(v, k->_bow_vec);
        if (c > 0) want.push_back(KeyFrameDatabase::Hit{ k, c, Frame::_vocab->score(v, k->_bow_vec) });
    }
    std::sort(want.begin(), want.end(), [](const KeyFrameDatabase::Hit &a, const KeyFrameDatabase::Hit &b) { return a.kf->_keyframe_id < b.kf->_keyframe_id; });
    if (want.size() != hits.size()) return false;
    for (size_t i = 0; i < want.size(); ++i)
        if (want[i].kf != hits[i].kf || want[i].common != hits[i].common || !same_bits(want[i].score, hits[i].score)) return false;
    return true;
}

// mode 1: every keyframe; mode 2: every second one
void maybe_add(KeyFrameDatabase *db, int mode, Frame *kf)
{
    if (mode == 1 || (mode == 2 && kf->_keyframe_id % 2 == 0)) db->Add(kf);
}

size_t put_list(double *o, size_t at, size_t n, const vector<double> &v)
{
    o[at] = (double)v.size();
    for (size_t k = 0; k < n; ++k) o[at + 1 + k] = k < v.size() ? v[k] : -7.0;
    return at + 1 + n;
}
template <class T> vector<double> as_doubles(const vector<T> &v) { return vector<double>(v.begin(), v.end()); }
}

extern "C" {

// the arguments of loop_run (tests/cpp/loop_surface.cpp) and the mode.  Per call (revisit keyframes, then the other texture's), out [q][256]:
//   0 DetectLoop, 1 ComputeSim3 (0 when not called), 2 matched keyframe id (-1), 3..10 S12, 11..18 corrected pose, 19 GetMatches size,
//   20 Stats::min_score, then seven lists as (size, 16 values padded with -7): candidates, acc_scores, consistency, consistent, bow_pairs,
//   ransac_inliers, refined_inliers (21 .. 139); 200 keyframe id, 201 hits of the Query, 202 Query equals the host functions (modes 1, 2),
//   203 keyframes the database holds.
// checks [16] (mode 1; all must be 1): 0 Add(nullptr) false, 1 Add of a held keyframe false, 2 Add of a bad keyframe false, 3 Add of a keyframe
//   without words false, 4 Erase of one not held false, 5 Erase of a held one true and Has false, 6 Add again true and Has true, 7 Size as
//   counted, 8 the batch Query of 70 vectors equals 70 single ones, 9 a query after Erase leaves the keyframe out, 10 Clear empties, 11 an empty
//   database answers true with no hits.
// Returns 0, 1 on an exception, 2 when the vocabulary does not load.
int kfdb_loop_run(int w, int h, const uint8_t *old_bgr, const float *old_depth, const double *old_T, int n_old, const uint8_t *lead_bgr,
                  const float *lead_depth, const double *lead_T, const uint8_t *rev_bgr, const float *rev_depth, const double *rev_T, int n_rev,
                  const double *drift, const uint8_t *oth_bgr, const float *oth_depth, const double *oth_T, int n_oth, int min_kf_gap,
                  int consistency_th, const void *vocab, size_t vocab_bytes, int mode, double *out, double *checks)
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
        {
            Scene s{ w, h, &cam, &detector, {}, {} };
            KeyFrameDatabase db;
            const size_t fb = (size_t)w * h * 3, db_ = (size_t)w * h;
            const Sim3 I, D = Sim3::from8(drift);
            vector<Frame *> old;
            for (int k = 0; k < n_old; ++k) {
                old.push_back(make_keyframe(s, old_bgr + k * fb, old_depth + k * db_, old_T + 7 * k, I));
                maybe_add(&db, mode, old.back());
            }
            for (int i = 0; i < n_old; ++i)
                for (int j = i + 1; j < n_old && j <= i + 2; ++j) link_keyframes(old[i], old[j], 100 - 20 * (j - i));
            for (Frame *kf : old) kf->UpdateBestCovisibles();
            vector<Frame *> rev;
            rev.push_back(make_keyframe(s, lead_bgr, lead_depth, lead_T, D));
            maybe_add(&db, mode, rev.back());
            auto one_call = [&](LoopClosing &L, Frame *kf, double *o) {
                for (int k = 0; k < 256; ++k) o[k] = 0;
                const vector<Frame *> all = s.kfs;
                const bool det = L.DetectLoop(kf, all);
                const bool ok = det && L.ComputeSim3();
                o[0] = det; o[1] = ok;
                o[2] = L.GetMatchedKeyframe() ? (double)L.GetMatchedKeyframe()->_keyframe_id : -1.0;
                L.GetSim3().to8(o + 3);
                L.GetCorrectedPose().to8(o + 11);
                o[19] = (double)L.GetMatches().size();
                const LoopClosing::Stats &st = L.GetStats();
                o[20] = st.min_score;
                size_t at = 21;
                at = put_list(o, at, 16, as_doubles(st.candidates));
                at = put_list(o, at, 16, st.acc_scores);
                at = put_list(o, at, 16, as_doubles(st.consistency));
                at = put_list(o, at, 16, as_doubles(st.consistent));
                at = put_list(o, at, 16, as_doubles(st.bow_pairs));
                at = put_list(o, at, 16, as_doubles(st.ransac_inliers));
                at = put_list(o, at, 16, as_doubles(st.refined_inliers));
                o[200] = (double)kf->_keyframe_id;
                if (mode != 0) {
                    vector<KeyFrameDatabase::Hit> hits;
                    const bool q = db.Query(kf->_bow_vec, hits);
                    o[201] = (double)hits.size();
                    o[202] = q && query_equals_host(db, kf->_bow_vec, all, hits);
                    o[203] = (double)db.Size();
                }
            };
            LoopClosing lc, lo;
            for (LoopClosing *l : { &lc, &lo }) {
                l->_option._min_kf_gap = min_kf_gap; l->_option._consistency_th = consistency_th;
                if (mode != 0) l->SetKeyFrameDatabase(&db);
            }
            int q = 0;
            for (int k = 0; k < n_rev; ++k, ++q) {
                Frame *kf = make_keyframe(s, rev_bgr + k * fb, rev_depth + k * db_, rev_T + 7 * k, D);
                maybe_add(&db, mode, kf);
                for (Frame *r : rev) link_keyframes(kf, r, 50);
                rev.push_back(kf);
                for (Frame *r : rev) { r->_cov_keyframes.clear(); r->_cov_weights.clear(); r->UpdateBestCovisibles(); }
                one_call(lc, kf, out + 256 * (size_t)q);
            }
            vector<Frame *> oth;
            for (int k = 0; k < n_oth; ++k, ++q) {
                Frame *kf = make_keyframe(s, oth_bgr + k * fb, oth_depth + k * db_, oth_T + 7 * k, I);
                maybe_add(&db, mode, kf);
                for (Frame *r : oth) link_keyframes(kf, r, 50);
                oth.push_back(kf);
                one_call(lo, kf, out + 256 * (size_t)q);
            }
            if (mode == 1 && checks) {
                for (int k = 0; k < 16; ++k) checks[k] = 0;
                Frame *a = s.kfs[3], *b = s.kfs[7];
                const size_t n0 = db.Size();
                checks[0] = !db.Add(nullptr);
                checks[1] = !db.Add(a) && db.Size() == n0;
                checks[5] = db.Erase(b) && !db.Has(b) && db.Size() == n0 - 1;
                checks[4] = !db.Erase(b) && !db.Erase(nullptr);
                b->_bad = true;
                checks[2] = !db.Add(b) && !db.Has(b);
                b->_bad = false;
                Frame empty;
                checks[3] = !db.Add(&empty) && !db.Has(&empty) && db.Size() == n0 - 1;
                vector<KeyFrameDatabase::Hit> hits;
                bool left_out = db.Query(a->_bow_vec, hits) && query_equals_host(db, a->_bow_vec, s.kfs, hits);
                for (const KeyFrameDatabase::Hit &x : hits) left_out = left_out && x.kf != b;
                checks[9] = left_out;
                checks[6] = db.Add(b) && db.Has(b);
                checks[7] = db.Size() == n0 && n0 == s.kfs.size();
                vector<const DBoW3::BowVector *> vs;
                for (int k = 0; k < 70; ++k) vs.push_back(&s.kfs[(size_t)k % s.kfs.size()]->_bow_vec);
                vector<vector<KeyFrameDatabase::Hit>> many;
                bool batch = db.Query(vs, many) && many.size() == vs.size();
                for (size_t k = 0; batch && k < vs.size(); ++k) batch = query_equals_host(db, *vs[k], s.kfs, many[k]) && !many[k].empty();
                checks[8] = batch;
                db.Clear();
                checks[10] = db.Size() == 0 && !db.Has(a);
                checks[11] = db.Query(a->_bow_vec, hits) && hits.empty();
                checks[10] = checks[10] && db.Add(a) && db.Query(a->_bow_vec, hits) && hits.size() == 1 && hits[0].kf == a;
            }
            for (Frame *kf : s.kfs) delete kf;
            for (MapPoint *mp : s.mps) delete mp;
        }
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
    } catch (const std::exception &e) {
        fprintf(stderr, "kfdb_loop_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

// the arguments of reloc_run (tests/cpp/reloc_surface.cpp) without the next frames, and the mode.  Per query q, out [q][40]:
//   0 ok, 1..7 T_cw after Relocalize (from identity), 8..11 stats (candidates, pnp_problems, ransac_inliers, final_inliers), 12 features,
//   13 matched keyframe id (-1), 14 bow_matches' size, 15..22 its values (-7 beyond), 30 Query of the frame's own BoW vector equals the host
//   functions (modes 1, 2), 31 its hits
int kfdb_reloc_run(int w, int h, const uint8_t *kf_bgr, const float *kf_depth, const double *T_kf, int n_kf, const uint8_t *q_bgr, int n_q,
                   const void *vocab, size_t vocab_bytes, int mode, double *out)
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
        {
            Scene s{ w, h, &cam, &detector, {}, {} };
            KeyFrameDatabase db;
            const size_t fb = (size_t)w * h * 3;
            const Sim3 I;
            for (int k = 0; k < n_kf; ++k) {
                Frame *kf = make_keyframe(s, kf_bgr + (size_t)k * fb, kf_depth + (size_t)k * w * h, T_kf + 7 * k, I);
                maybe_add(&db, mode, kf);
            }
            for (int q = 0; q < n_q; ++q) {
                double *o = out + 40 * (size_t)q;
                for (int k = 0; k < 40; ++k) o[k] = 0;
                Frame *cur = new Frame;
                cur->_id = 1000 + (unsigned long)q;
                cur->_color = cv::Mat(h, w, CV_8UC3, const_cast<uint8_t *>(q_bgr + (size_t)q * fb));
                cur->InitFrame();
                cur->_TCW = SE3();
                Relocalizer reloc;
                if (mode != 0) reloc.SetKeyFrameDatabase(&db);
                const bool ok = reloc.Relocalize(cur, s.kfs);
                double T[7]; cur->_TCW.to7(T);
                o[0] = ok;
                for (int k = 0; k < 7; ++k) o[1 + k] = T[k];
                const Relocalizer::Stats &st = reloc.GetStats();
                o[8] = st.candidates; o[9] = st.pnp_problems; o[10] = st.ransac_inliers; o[11] = st.final_inliers;
                o[12] = (double)cur->_features.size();
                o[13] = reloc.GetMatchedKeyframe() ? (double)reloc.GetMatchedKeyframe()->_keyframe_id : -1.0;
                put_list(o, 14, 8, as_doubles(st.bow_matches));
                if (mode != 0) {
                    // the frame's BoW vector again (Relocalize leaves it empty), asked directly
                    Frame *c2 = new Frame;
                    c2->_color = cur->_color;
                    c2->InitFrame();
                    detector.Detect(c2);
                    detector.ComputeAngleAndDescriptor(c2);
                    c2->ComputeBoW();
                    vector<KeyFrameDatabase::Hit> hits;
                    const bool qk = db.Query(c2->_bow_vec, hits);
                    o[30] = qk && !c2->_bow_vec.empty() && query_equals_host(db, c2->_bow_vec, s.kfs, hits);
                    o[31] = (double)hits.size();
                    delete c2;
                }
                delete cur;
            }
            for (Frame *kf : s.kfs) delete kf;
            for (MapPoint *mp : s.mps) delete mp;
        }
        Frame::SetORBVocabulary(nullptr);
        Memory::Clean();
    } catch (const std::exception &e) {
        fprintf(stderr, "kfdb_reloc_run: %s\n", e.what());
        return 1;
    }
    return 0;
}

// The parent's way, for tools/kfdb_bench.py: n_rows BoW vectors as std::map (rows by r_off into r_word / r_weight), one query vector; `reps`
// passes of common words + Vocabulary::score (L1: a default-constructed vocabulary) over every row on one host core.  Returns the median
// milliseconds of a pass; common / score [n_rows] of the last pass.
double kfdb_host_loop_ms(int n_rows, const int32_t *r_off, const int32_t *r_word, const double *r_weight, const int32_t *q_word,
                         const double *q_weight, int n_q, int reps, int32_t *common, double *score)
{
    vector<DBoW3::BowVector> rows((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r)
        for (int i = r_off[r]; i < r_off[r + 1]; ++i) rows[r][(DBoW3::WordId)r_word[i]] = r_weight[i];
    DBoW3::BowVector q;
    for (int i = 0; i < n_q; ++i) q[(DBoW3::WordId)q_word[i]] = q_weight[i];
    DBoW3::Vocabulary voc;
    vector<double> ms;
    for (int rep = 0; rep < reps; ++rep) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < n_rows; ++r) {
            common[r] = common_words(q, rows[r]);
            score[r] = voc.score(q, rows[r]);
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    return ms.empty() ? 0.0 : ms[ms.size() / 2];
}

}  // extern "C"
