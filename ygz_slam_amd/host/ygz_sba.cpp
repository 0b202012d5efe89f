// ygz::BundleAdjuster (include/ygz/Algorithm/BundleAdjuster.h): nothing in the reference.  ORB-SLAM2's Optimizer::LocalBundleAdjustment and
// GlobalBundleAdjustemnt with stereo edges as synchronous calls: keyframe poses, map points and their observations are gathered into one
// problem, one ygz_hip_stereo_ba call (ygz_slam_amd/csrc/sba.hip) optimises it and classifies every edge, poses and points are rewritten
// from its result and, for the local form, the outlier observations leave the map.  Every order ORB-SLAM2 leaves to set iteration over
// pointers goes by keyframe id or index here.  Not part of it: a background thread, covisibility upkeep after an erasure, killing points.
// Error conventions of the other surfaces: a failed call logs and returns false, only a missing device throws.
#include "ygz/Algorithm/BundleAdjuster.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <algorithm>

namespace ygz {

namespace {
bool by_id(const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; }

void sort_unique(vector<Frame *> &kfs)
{
    std::sort(kfs.begin(), kfs.end(), by_id);
    kfs.erase(std::unique(kfs.begin(), kfs.end()), kfs.end());
}
}

void BundleAdjuster::SetURight(const Frame *kf, const std::vector<double> &u_right) { if (kf) _u_right[kf->_keyframe_id] = u_right; }
void BundleAdjuster::ClearURight(const Frame *kf) { if (kf) _u_right.erase(kf->_keyframe_id); }
void BundleAdjuster::Clear() { _u_right.clear(); }

bool BundleAdjuster::GatherGlobal(const vector<Frame *> &keyframes)
{
    vector<Frame *> kfs;
    for (Frame *k : keyframes) if (k && !k->_bad) kfs.push_back(k);
    sort_unique(kfs);
    return Gather(kfs, false, "GlobalBundleAdjustment");
}

bool BundleAdjuster::GatherLocal(Frame *keyframe)
{
    vector<Frame *> kfs;
    if (keyframe && !keyframe->_bad) {
        kfs.push_back(keyframe);
        for (Frame *k : keyframe->_cov_keyframes) if (k && !k->_bad) kfs.push_back(k);
    }
    sort_unique(kfs);
    return Gather(kfs, true, "LocalBundleAdjustment");
}

// free_kfs: not bad, by id, once each.  local: every other keyframe that observes one of their points joins as a fixed pose
bool BundleAdjuster::Gather(const vector<Frame *> &free_kfs, bool local, const char *who)
{
    _problem = Problem();
    _result = Result();
    _outlier_count = 0;
    _kfs.clear(); _pts.clear(); _edge_feat.clear();
    Problem &g = _problem;
    const PinholeCamera *cam = Frame::GetCamera();
    if (free_kfs.empty() || !cam) {
        LOG(ERROR) << "BundleAdjuster::" << who << ": no keyframe or no camera: nothing to adjust" << endl;
        return false;
    }
    // the points: the good map points of the free keyframes' features, each once, keyframes by id, features by index
    vector<MapPoint *> cand;
    std::set<MapPoint *> seen;
    for (Frame *k : free_kfs)
        for (Feature *f : k->_features) {
            MapPoint *mp = f ? f->_mappoint : nullptr;
            if (mp && !mp->_bad && seen.insert(mp).second) cand.push_back(mp);
        }
    // the poses, by id: the free keyframes and, for the local form, every other keyframe that is not bad in those points' observations
    std::set<const Frame *> is_free(free_kfs.begin(), free_kfs.end());
    vector<Frame *> kfs = free_kfs;
    if (local) {
        for (MapPoint *mp : cand)
            for (const auto &ob : mp->_obs) {
                Frame *o = ob.second ? ob.second->_frame : nullptr;
                if (o && !o->_bad && !is_free.count(o)) kfs.push_back(o);
            }
        sort_unique(kfs);
    }
    const int N = (int)kfs.size();
    if (N < 2) {
        LOG(ERROR) << "BundleAdjuster::" << who << ": " << N << " keyframes: nothing to adjust" << endl;
        return false;
    }
    map<const Frame *, int> pose_of;
    vector<map<const Feature *, int>> index_of(N);
    for (int v = 0; v < N; ++v) {
        pose_of[kfs[v]] = v;
        for (size_t i = 0; i < kfs[v]->_features.size(); ++i) index_of[v][kfs[v]->_features[i]] = (int)i;
    }
    g.fixed.assign(N, 0);
    if ((int)free_kfs.size() == N) g.fixed[0] = 1;                     // no fixed keyframe: the free one of smallest id
    else for (int v = 0; v < N; ++v) g.fixed[v] = is_free.count(kfs[v]) ? 0 : 1;

    // the edges, per point in the key order of its observations; points with fewer than two edges are left out
    vector<int> degree(N, 0);
    struct E1 { int pose, feature; Feature *f; };
    for (MapPoint *mp : cand) {
        vector<E1> edges;
        for (const auto &ob : mp->_obs) {
            Feature *f = ob.second;
            if (!f || !f->_frame) continue;
            auto it = pose_of.find(f->_frame);
            if (it == pose_of.end()) continue;
            auto ix = index_of[it->second].find(f);
            if (ix == index_of[it->second].end()) continue;            // not a feature of its frame
            edges.push_back(E1{ it->second, ix->second, f });
        }
        if (edges.size() < 2) { ++g.points_left_out; continue; }
        const int l = (int)_pts.size();
        _pts.push_back(mp);
        g.point_ids.push_back(mp->_id);
        for (int k = 0; k < 3; ++k) g.points.push_back(mp->_pos_world[k]);
        for (const E1 &e : edges) {
            double ur = -1.0;
            auto u = _u_right.find(kfs[e.pose]->_keyframe_id);
            if (u != _u_right.end() && (size_t)e.feature < u->second.size()) ur = u->second[e.feature];
            const bool stereo = ur >= 0;
            g.edge_pose.push_back(e.pose); g.edge_point.push_back(l); g.edge_feature.push_back(e.feature);
            g.obs.push_back(e.f->_pixel[0]); g.obs.push_back(e.f->_pixel[1]); g.obs.push_back(stereo ? ur : 0.0);
            g.kind.push_back(stereo ? 2 : 1); g.level.push_back(e.f->_level);
            _edge_feat.push_back(e.f);
            ++degree[e.pose];
        }
    }
    const int L = (int)_pts.size(), E = (int)g.edge_pose.size();
    for (int v = 0; v < N; ++v)
        if (!g.fixed[v] && !degree[v]) {
            LOG(ERROR) << "BundleAdjuster::" << who << ": keyframe " << kfs[v]->_keyframe_id << " shares no map point with the others" << endl;
            return false;
        }
    if (L < 1 || N > YGZ_GBA_MAX_POSES || L > YGZ_GBA_MAX_POINTS || E > YGZ_GBA_MAX_EDGES) {
        LOG(ERROR) << "BundleAdjuster::" << who << ": " << N << " keyframes, " << L << " points, " << E << " observations: outside the solver's range" << endl;
        return false;
    }
    g.poses.resize((size_t)N * 7);
    for (int v = 0; v < N; ++v) {
        g.keyframe_ids.push_back(kfs[v]->_keyframe_id);
        kfs[v]->_TCW.to7(&g.poses[(size_t)v * 7]);
    }
    g.K4[0] = cam->fx(); g.K4[1] = cam->fy(); g.K4[2] = cam->cx(); g.K4[3] = cam->cy();
    _kfs = kfs;
    return true;
}

// one ygz_hip_stereo_ba call on the gathered problem; on success the free poses and the points are rewritten
bool BundleAdjuster::Solve(int rounds, int robust_rounds, const int *iterations, const char *who)
{
    Problem &g = _problem;
    const int N = (int)_kfs.size(), L = (int)_pts.size(), E = (int)g.edge_pose.size();
    ygz_sba_params prm;
    ygz_hip_default_sba_params(&prm);
    prm.max_trials = _options._max_trials; prm.cg_max_iterations = _options._cg_max_iterations; prm.cg_batch = _options._cg_batch;
    prm.cg_tol = _options._cg_tol; prm.min_rel_decrease = _options._min_rel_decrease;
    prm.baseline = _options._baseline; prm.chi2_mono = _options._chi2_mono; prm.chi2_stereo = _options._chi2_stereo;
    prm.rounds = rounds; prm.robust_rounds = robust_rounds;
    for (int k = 0; k < YGZ_SBA_MAX_ROUNDS; ++k) prm.iterations[k] = k < rounds && k < 4 ? iterations[k] : 0;
    ygz_sba_result res;
    g.poses_out.assign((size_t)N * 7, 0.0); g.points_out.assign((size_t)L * 3, 0.0); g.outlier.assign(E, 0); g.chi2.assign(E, 0.0);
    if (!hip::check(ygz_hip_stereo_ba(hip::Runtime::Get().ctx(), N, g.poses.data(), g.fixed.data(), L, g.points.data(), E, g.edge_pose.data(),
                                      g.edge_point.data(), g.obs.data(), g.kind.data(), g.level.data(), g.K4, &prm, g.poses_out.data(),
                                      g.points_out.data(), g.outlier.data(), g.chi2.data(), &res), "stereo_ba")) {
        g.poses_out.clear(); g.points_out.clear(); g.outlier.clear(); g.chi2.clear();
        return false;
    }
    _result._rounds_run = res.rounds_run; _result._launches = res.launches;
    for (int k = 0; k < 4; ++k) {
        Round &r = _result._rounds[k];
        r._status = res.status[k]; r._lm_iterations = res.lm_iterations[k]; r._n_solves = res.n_solves[k]; r._cg_iterations = res.cg_iterations[k];
        r._cg_capped = res.cg_capped[k]; r._inliers = res.inliers[k]; r._cost_initial = res.cost_initial[k]; r._cost_final = res.cost_final[k];
        r._lambda = res.lambda[k];
    }
    for (uint8_t o : g.outlier) _outlier_count += o ? 1 : 0;
    if (res.status[0] == YGZ_GBA_FAILED) {
        LOG(ERROR) << "BundleAdjuster::" << who << ": a map point is not in front of one of its keyframes" << endl;
        return false;
    }
    for (int v = 0; v < N; ++v)
        if (!g.fixed[v]) _kfs[v]->_TCW = SE3::from7(&g.poses_out[(size_t)v * 7]);
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < 3; ++k) _pts[l]->_pos_world[k] = g.points_out[(size_t)l * 3 + k];
    return true;
}

int BundleAdjuster::EraseOutliers(const std::vector<uint8_t> &outlier)
{
    if (outlier.size() != _edge_feat.size()) return 0;
    int erased = 0;
    for (size_t e = 0; e < outlier.size(); ++e) {
        if (!outlier[e]) continue;
        Feature *f = _edge_feat[e];
        MapPoint *mp = _pts[_problem.edge_point[e]];
        auto it = mp->_obs.find(_kfs[_problem.edge_pose[e]]->_keyframe_id);
        if (it != mp->_obs.end() && it->second == f) { mp->_obs.erase(it); ++erased; }
        if (f->_mappoint == mp) f->_mappoint = nullptr;
    }
    return erased;
}

bool BundleAdjuster::GlobalBundleAdjustment(const vector<Frame *> &keyframes)
{
    if (!GatherGlobal(keyframes)) return false;
    const int it[4] = { _options._gba_iterations, 0, 0, 0 };
    return Solve(1, 1, it, "GlobalBundleAdjustment");
}

bool BundleAdjuster::LocalBundleAdjustment(Frame *keyframe)
{
    if (!GatherLocal(keyframe)) return false;
    if (!Solve(_options._rounds, _options._robust_rounds, _options._iterations, "LocalBundleAdjustment")) return false;
    if (_options._erase_outliers) EraseOutliers(_problem.outlier);
    return true;
}

}  // namespace ygz
