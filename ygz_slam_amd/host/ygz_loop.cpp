// ygz::LoopClosing (include/ygz/Algorithm/LoopClosing.h): nothing in the reference -- LocalMapping.cpp:330 leaves loop detection as a comment.
// The rules are ORB-SLAM2's LoopClosing::DetectLoop and KeyFrameDatabase::DetectLoopCandidates over the keyframes' BoW vectors and covisibility,
// with every tie broken by keyframe id; the geometric check of all candidates is one ygz_hip_sim3_ransac call (ygz_slam_amd/csrc/sim3.hip).
// Error conventions of the other surfaces: a failed call logs and returns false, only a missing device throws.
#include "ygz/Algorithm/LoopClosing.h"
#include "ygz/Algorithm/KeyFrameDatabase.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <algorithm>

namespace ygz {

namespace {
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

bool ensure_bow(Frame *kf)
{
    if (kf->_bow_vec.empty()) kf->ComputeBoW();
    return !kf->_bow_vec.empty();
}

// the connected keyframes that are not bad, heaviest first, equal weights by keyframe id (independent of addresses)
vector<Frame *> best_covisibles(const Frame *kf, int n)
{
    vector<pair<int, Frame *>> wk;
    for (const auto &c : kf->_connected_keyframe_weights)
        if (c.first && !c.first->_bad) wk.push_back(make_pair(c.second, c.first));
    std::sort(wk.begin(), wk.end(), [](const pair<int, Frame *> &a, const pair<int, Frame *> &b) {
        return a.first != b.first ? a.first > b.first : a.second->_keyframe_id < b.second->_keyframe_id; });
    vector<Frame *> out;
    for (const auto &p : wk) {
        if ((int)out.size() >= n) break;
        out.push_back(p.second);
    }
    return out;
}

struct Problem {
    Frame *kf;
    size_t cand;                                      // index into the enough-consistent candidates
    vector<pair<Feature *, Feature *>> pairs;         // (current feature, candidate feature), both with a good map point
    ygz_sim3_result res;
    size_t first = 0;
};
}

bool LoopClosing::DetectLoop(Frame *kf)
{
    vector<Frame *> kfs;
    const int n = Memory::GetNumberFrames();
    for (int id = 0; id < n; ++id) {
        Frame *k = Memory::GetKeyFrame((unsigned long)id);
        if (k) kfs.push_back(k);
    }
    return DetectLoop(kf, kfs);
}

bool LoopClosing::DetectLoop(Frame *kf, const vector<Frame *> &keyframes)
{
    _stats = Stats();
    _enough_consistent.clear();
    _acc_score.clear();
    _current = nullptr;
    _searched = _fusable = false;
    if (!kf || Frame::_vocab == nullptr) {
        LOG(ERROR) << "LoopClosing::DetectLoop: no keyframe or no vocabulary" << endl;
        return false;
    }
    // 1. too close to the last loop (or to the start of the map): nothing, the consistency state is left alone
    if (kf->_keyframe_id < _last_loop_kf_id + (unsigned long)std::max(0, _option._min_kf_gap)) return false;
    if (!ensure_bow(kf)) {
        _consistent_groups.clear();
        return false;
    }
    // an attached database answers steps 2 and 3 for the keyframes it holds with one device query: the same numbers (KeyFrameDatabase.h)
    map<const Frame *, KeyFrameDatabase::Hit> db_hit;
    vector<KeyFrameDatabase::Hit> hits;
    const bool from_db = _kfdb && Frame::_vocab->scoring_ == 0 && _kfdb->Query(kf->_bow_vec, hits);
    for (const KeyFrameDatabase::Hit &h : hits) db_hit[h.kf] = h;
    // held and scored by the query: a keyframe that is not among the hits shares no word, and Vocabulary::score returns -0.0 / 2 for it
    auto db_answer = [&](Frame *k, int &common, double &score) {
        if (!from_db || !_kfdb->Has(k)) return false;
        auto it = db_hit.find(k);
        common = it != db_hit.end() ? it->second.common : 0;
        score = it != db_hit.end() ? it->second.score : -0.0 / 2.0;
        return true;
    };
    // 2. minScore: the lowest score against the connected keyframes (1 without any)
    double min_score = 1.0;
    for (const auto &c : kf->_connected_keyframe_weights) {
        Frame *n = c.first;
        if (!n || n->_bad || n == kf || !ensure_bow(n)) continue;
        int cn = 0;
        double sn = 0;
        if (!db_answer(n, cn, sn)) sn = Frame::_vocab->score(kf->_bow_vec, n->_bow_vec);
        min_score = std::min(min_score, sn);
    }
    _stats.min_score = min_score;

    // 3. keyframes sharing words, not kf, not bad, not connected to kf; above the common-words floor, then scored against minScore
    vector<pair<Frame *, int>> sharing;
    int max_common = 0;
    for (Frame *k : keyframes) {
        if (!k || k == kf || k->_bad || kf->_connected_keyframe_weights.count(k)) continue;
        if (!ensure_bow(k)) continue;
        int c = 0;
        double sk = 0;
        if (!db_answer(k, c, sk)) c = common_words(kf->_bow_vec, k->_bow_vec);
        if (c <= 0) continue;
        sharing.push_back(make_pair(k, c));
        max_common = std::max(max_common, c);
    }
    map<Frame *, double> passed;                                      // keyframe -> score (step 3 passed)
    const double min_common = _option._min_common_words_ratio * max_common;
    for (const auto &s : sharing) {
        if (!(s.second > min_common)) continue;
        int cs = 0;
        double si = 0;
        if (!db_answer(s.first, cs, si)) si = Frame::_vocab->score(kf->_bow_vec, s.first->_bow_vec);
        if (si >= min_score) passed[s.first] = si;
    }

    // 4. group scores over the best covisibles that passed too; the representative is the group's best (ties: smaller id)
    vector<pair<Frame *, double>> groups;                             // representative, accScore
    double best_acc = 0.0;
    for (const auto &p : passed) {
        Frame *best = p.first;
        double best_score = p.second, acc = p.second;
        for (Frame *n : best_covisibles(p.first, _option._acc_covisibles)) {
            auto it = passed.find(n);
            if (it == passed.end()) continue;
            acc += it->second;
            if (it->second > best_score || (it->second == best_score && n->_keyframe_id < best->_keyframe_id)) { best = n; best_score = it->second; }
        }
        groups.push_back(make_pair(best, acc));
        best_acc = std::max(best_acc, acc);
    }
    map<unsigned long, Frame *> cands;                                // by keyframe id, once each
    for (const auto &g : groups) {
        if (!(g.second > _option._acc_score_ratio * best_acc)) continue;
        if (!cands.count(g.first->_keyframe_id)) { cands[g.first->_keyframe_id] = g.first; _acc_score[g.first->_keyframe_id] = g.second; }
        else _acc_score[g.first->_keyframe_id] = std::max(_acc_score[g.first->_keyframe_id], g.second);
    }
    for (const auto &c : cands) { _stats.candidates.push_back(c.first); _stats.acc_scores.push_back(_acc_score[c.first]); }
    if (cands.empty()) {
        _consistent_groups.clear();
        return false;
    }

    // 5. consistency with the previous call's groups
    vector<ConsistentGroup> current;
    vector<char> extended(_consistent_groups.size(), 0);
    for (const auto &c : cands) {
        Frame *cand = c.second;
        std::set<unsigned long> group;
        group.insert(cand->_keyframe_id);
        for (const auto &n : cand->_connected_keyframe_weights) if (n.first) group.insert(n.first->_keyframe_id);
        bool enough = false, some = false;
        int consistency = 0;
        for (size_t g = 0; g < _consistent_groups.size(); ++g) {
            const std::set<unsigned long> &prev = _consistent_groups[g].first;
            bool hit = false;
            for (unsigned long id : group) if (prev.count(id)) { hit = true; break; }
            if (!hit) continue;
            some = true;
            const int cur = _consistent_groups[g].second + 1;
            consistency = std::max(consistency, cur);
            if (!extended[g]) { current.push_back(make_pair(group, cur)); extended[g] = 1; }
            if (cur >= _option._consistency_th && !enough) { _enough_consistent.push_back(cand); enough = true; }
        }
        if (!some) current.push_back(make_pair(group, 0));
        _stats.consistency.push_back(consistency);
    }
    _consistent_groups = current;
    for (Frame *c : _enough_consistent) _stats.consistent.push_back(c->_keyframe_id);
    // 6. the enough-consistent candidates wait for ComputeSim3
    if (_enough_consistent.empty()) return false;
    _current = kf;
    return true;
}

bool LoopClosing::ComputeSim3()
{
    _matched = nullptr;
    _correctable = false;
    _searched = _fusable = false;
    _S12 = Sim3(); _Scw = Sim3();
    _matches.clear();
    _stats.bow_pairs.clear(); _stats.ransac_inliers.clear(); _stats.refined_inliers.clear();
    Frame *kf = _current;
    if (!kf || _enough_consistent.empty() || Frame::GetCamera() == nullptr) return false;

    // 1-2. SearchByBoW against each candidate; pairs whose features both have a good map point, each map point once on each side
    _matcher._options.knnRatio = _option._knn_ratio;
    vector<Problem> probs;
    for (size_t ci = 0; ci < _enough_consistent.size(); ++ci) {
        Frame *cand = _enough_consistent[ci];
        _stats.ransac_inliers.push_back(-1);
        _stats.refined_inliers.push_back(-1);
        Problem pb;
        pb.kf = cand; pb.cand = ci;
        if (!cand->_bad && ensure_bow(cand)) {
            map<int, int> m;
            _matcher.SearchByBoW(kf, cand, m);
            std::set<MapPoint *> used1, used2;
            for (const auto &ij : m) {
                if (ij.first < 0 || ij.first >= (int)kf->_features.size() || ij.second < 0 || ij.second >= (int)cand->_features.size()) continue;
                Feature *f1 = kf->_features[ij.first], *f2 = cand->_features[ij.second];
                MapPoint *p1 = f1->_mappoint, *p2 = f2->_mappoint;
                if (!p1 || !p2 || p1->_bad || p2->_bad || used1.count(p1) || used2.count(p2)) continue;
                used1.insert(p1); used2.insert(p2);
                pb.pairs.push_back(make_pair(f1, f2));
            }
        }
        _stats.bow_pairs.push_back((int)pb.pairs.size());
        if ((int)pb.pairs.size() >= std::max(_option._min_bow_matches, 3) && (int)probs.size() < YGZ_SIM3_MAX_PROBLEMS) probs.push_back(std::move(pb));
    }
    if (probs.empty()) return false;

    // 3. every candidate through one Sim3 RANSAC call: X1 = T_1w P1, X2 = T_2w P2
    vector<int32_t> off(1, 0), lv;
    vector<double> X1, X2, px1, px2;
    for (Problem &pb : probs) {
        pb.first = lv.size() / 2;
        for (const auto &fp : pb.pairs) {
            const Vector3d a = kf->_TCW * fp.first->_mappoint->_pos_world, b = pb.kf->_TCW * fp.second->_mappoint->_pos_world;
            for (int k = 0; k < 3; ++k) { X1.push_back(a[k]); X2.push_back(b[k]); }
            for (int k = 0; k < 2; ++k) { px1.push_back(fp.first->_pixel[k]); px2.push_back(fp.second->_pixel[k]); }
            lv.push_back(std::max(fp.first->_level, 0)); lv.push_back(std::max(fp.second->_level, 0));
        }
        off.push_back((int32_t)(lv.size() / 2));
    }
    const Matrix3d K = Frame::GetCamera()->GetCameraMatrix();
    const double K4[4] = { K(0, 0), K(1, 1), K(0, 2), K(1, 2) };
    ygz_sim3_params prm;
    ygz_hip_default_sim3_params(&prm);
    prm.max_iter = _option._ransac_iterations; prm.chi2 = _option._ransac_chi2; prm.min_inliers = _option._min_inliers;
    prm.chi2_refine = _option._refine_chi2; prm.fix_scale = _option._fix_scale ? 1 : 0;
    vector<ygz_sim3_result> res(probs.size());
    vector<uint8_t> mask(lv.size() / 2);
    if (!hip::check(ygz_hip_sim3_ransac(hip::Runtime::Get().ctx(), (int)probs.size(), off.data(), X1.data(), X2.data(), px1.data(), px2.data(),
                                        lv.data(), K4, &prm, res.data(), mask.data()), "sim3_ransac"))
        return false;
    for (size_t p = 0; p < probs.size(); ++p) {
        probs[p].res = res[p];
        _stats.ransac_inliers[probs[p].cand] = res[p].n_inliers;
        _stats.refined_inliers[probs[p].cand] = res[p].n_refined;
    }

    // 4. the candidate with the most refined inliers (ties: group score, then keyframe id) among the successful ones
    const Problem *best = nullptr;
    for (const Problem &pb : probs) {
        if (!pb.res.success) continue;
        if (!best) { best = &pb; continue; }
        const double a = _acc_score[pb.kf->_keyframe_id], b = _acc_score[best->kf->_keyframe_id];
        if (pb.res.n_refined > best->res.n_refined || (pb.res.n_refined == best->res.n_refined && (a > b || (a == b && pb.kf->_keyframe_id < best->kf->_keyframe_id))))
            best = &pb;
    }
    if (!best) return false;
    _matched = best->kf;
    _S12 = Sim3::from8(best->res.S12);
    _Scw = _S12 * best->kf->_TCW;
    for (size_t k = 0; k < best->pairs.size(); ++k)
        if (mask[best->first + k] & 2) _matches.push_back(make_pair(best->pairs[k].first->_mappoint, best->pairs[k].second->_mappoint));
    _last_loop_kf_id = kf->_keyframe_id;
    _correctable = true;
    return true;
}

// ORB-SLAM2 LoopClosing::ComputeSim3's second half.  (Re-running the 7-dof refinement on the widened pairs, as ORB-SLAM2 does between the two
// searches, needs a refine-only entry of the C ABI: not here, S12 stays the one ComputeSim3 found.)
bool LoopClosing::SearchLoopMapPoints()
{
    _current_matched.clear();
    _loop_points.clear();
    _searched = _fusable = false;                                    // FuseLoop works on this call's vectors
    _stats.sim3_added = _stats.projection_added = _stats.total_matches = 0;
    Frame *kf = _current;
    if (!kf || !_matched || _matches.empty()) return false;
    // 1. the refined inlier pairs, per feature of the current keyframe
    _current_matched.assign(kf->_features.size(), nullptr);
    map<const MapPoint *, MapPoint *> loop_of;
    for (const auto &m : _matches) loop_of[m.first] = m.second;
    for (size_t i = 0; i < kf->_features.size(); ++i) {
        auto it = loop_of.find(kf->_features[i]->_mappoint);
        if (kf->_features[i]->_mappoint && it != loop_of.end()) _current_matched[i] = it->second;
    }
    // 2. more pairs with the loop keyframe itself, by mutual projection with S12
    _stats.sim3_added = _matcher.SearchBySim3(kf, _matched, _current_matched, _S12, _option._sim3_search_th);
    // 3. the loop map points: the matched keyframe and its connected keyframes by keyframe id, features by index, each point once
    vector<Frame *> group(1, _matched);
    for (const auto &c : _matched->_connected_keyframe_weights)
        if (c.first && !c.first->_bad && c.first != _matched) group.push_back(c.first);
    std::sort(group.begin(), group.end(), [](const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; });
    std::set<MapPoint *> seen;
    for (Frame *g : group)
        for (Feature *f : g->_features) {
            MapPoint *mp = f->_mappoint;
            if (!mp || mp->_bad || !seen.insert(mp).second) continue;
            _loop_points.push_back(mp);
        }
    // 4. pulled into the current keyframe with the corrected pose
    _stats.projection_added = _matcher.SearchByProjection(kf, _Scw, _loop_points, _current_matched, _option._projection_search_th);
    // 5. enough matches in total
    for (const MapPoint *mp : _current_matched) if (mp) ++_stats.total_matches;
    _searched = _correctable;                                         // after the correction the revisit run's camera frames are rescaled
    return _stats.total_matches >= _option._min_total_matches;
}

}  // namespace ygz
