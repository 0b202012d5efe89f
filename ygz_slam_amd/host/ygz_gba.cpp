// ygz::LoopClosing::GlobalBundleAdjustment (include/ygz/Algorithm/LoopClosing.h): nothing in the reference, whose loop closing is empty.  What
// ORB-SLAM2's LoopClosing::CorrectLoop ends with, RunGlobalBundleAdjustment -> Optimizer::GlobalBundleAdjustemnt, as a synchronous call: the
// keyframes' poses and the map points they share are gathered into one problem, one ygz_hip_global_ba call (ygz_slam_amd/csrc/gba.hip)
// optimises it, poses and points are rewritten from its result.  Every order ORB-SLAM2 leaves to set iteration over pointers goes by keyframe
// id or index here.  Not part of it: the background thread and the propagation to keyframes created meanwhile, outlier culling, per-level
// information matrices.  Error conventions of the other surfaces: a failed call logs and returns false, only a missing device throws.
#include "ygz/Algorithm/LoopClosing.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <algorithm>

namespace ygz {

namespace {
bool by_id(const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; }
}

bool LoopClosing::GlobalBundleAdjustment()
{
    vector<Frame *> kfs;
    const int n = Memory::GetNumberFrames();
    for (int id = 0; id < n; ++id) {
        Frame *k = Memory::GetKeyFrame((unsigned long)id);
        if (k) kfs.push_back(k);
    }
    return GlobalBundleAdjustment(kfs);
}

bool LoopClosing::GlobalBundleAdjustment(const vector<Frame *> &keyframes)
{
    Stats::GlobalBAResult none;
    _stats.gba_poses = _stats.gba_points = _stats.gba_edges = _stats.gba_points_left_out = 0;
    _stats.global_ba = none;

    // 1. the poses: not bad, once each, by id; the first is fixed
    vector<Frame *> kfs;
    for (Frame *k : keyframes) if (k && !k->_bad) kfs.push_back(k);
    std::sort(kfs.begin(), kfs.end(), by_id);
    kfs.erase(std::unique(kfs.begin(), kfs.end()), kfs.end());
    const int N = (int)kfs.size();
    if (N < 2 || !Frame::GetCamera()) {
        LOG(ERROR) << "LoopClosing::GlobalBundleAdjustment: " << N << " keyframes: nothing to adjust" << endl;
        return false;
    }
    map<const Frame *, int> pose_of;
    for (int v = 0; v < N; ++v) pose_of[kfs[v]] = v;

    // 2. the points and their edges, 3. points with fewer than two edges are left out
    BundleProblem g;
    vector<MapPoint *> pts;
    std::set<MapPoint *> seen;
    vector<int> degree(N, 0);
    for (int v = 0; v < N; ++v)
        for (Feature *f : kfs[v]->_features) {
            MapPoint *mp = f ? f->_mappoint : nullptr;
            if (!mp || mp->_bad || !seen.insert(mp).second) continue;
            vector<pair<int, const Feature *>> edges;
            for (const auto &ob : mp->_obs) {                          // key order
                if (!ob.second || !ob.second->_frame) continue;
                auto it = pose_of.find(ob.second->_frame);
                if (it != pose_of.end()) edges.push_back(make_pair(it->second, (const Feature *)ob.second));
            }
            if (edges.size() < 2) { ++_stats.gba_points_left_out; continue; }
            const int l = (int)pts.size();
            pts.push_back(mp);
            g.point_ids.push_back(mp->_id);
            for (int k = 0; k < 3; ++k) g.points.push_back(mp->_pos_world[k]);
            for (const auto &e : edges) {
                g.edge_pose.push_back(e.first); g.edge_point.push_back(l);
                g.obs.push_back(e.second->_pixel[0]); g.obs.push_back(e.second->_pixel[1]);
                ++degree[e.first];
            }
        }
    const int L = (int)pts.size(), E = (int)g.edge_pose.size();
    _stats.gba_poses = N; _stats.gba_points = L; _stats.gba_edges = E;
    // 4. a free pose without an edge
    for (int v = 1; v < N; ++v)
        if (!degree[v]) {
            LOG(ERROR) << "LoopClosing::GlobalBundleAdjustment: keyframe " << kfs[v]->_keyframe_id << " shares no map point with the others" << endl;
            return false;
        }
    if (L < 1 || N > YGZ_GBA_MAX_POSES || L > YGZ_GBA_MAX_POINTS || E > YGZ_GBA_MAX_EDGES) {
        LOG(ERROR) << "LoopClosing::GlobalBundleAdjustment: " << N << " keyframes, " << L << " points, " << E << " observations: outside the solver's range" << endl;
        return false;
    }
    g.poses.resize((size_t)N * 7); g.fixed.assign(N, 0);
    g.fixed[0] = 1;
    for (int v = 0; v < N; ++v) {
        g.keyframe_ids.push_back(kfs[v]->_keyframe_id);
        kfs[v]->_TCW.to7(&g.poses[(size_t)v * 7]);
    }
    const PinholeCamera *cam = Frame::GetCamera();
    g.K4[0] = cam->fx(); g.K4[1] = cam->fy(); g.K4[2] = cam->cx(); g.K4[3] = cam->cy();
    g.huber_delta = _option._gba_huber_delta;

    // 5. one solver call
    ygz_gba_params prm;
    ygz_hip_default_gba_params(&prm);
    prm.max_iterations = _option._gba_iterations;
    ygz_gba_result res;
    g.poses_out.resize((size_t)N * 7); g.points_out.resize((size_t)L * 3);
    if (!hip::check(ygz_hip_global_ba(hip::Runtime::Get().ctx(), N, g.poses.data(), g.fixed.data(), L, g.points.data(), E, g.edge_pose.data(),
                                      g.edge_point.data(), g.obs.data(), g.K4, g.huber_delta, &prm, g.poses_out.data(), g.points_out.data(), &res),
                    "global_ba"))
        return false;
    Stats::GlobalBAResult &gr = _stats.global_ba;
    gr.status = res.status; gr.lm_iterations = res.lm_iterations; gr.n_solves = res.n_solves; gr.cg_iterations_total = res.cg_iterations_total;
    gr.cg_capped = res.cg_capped; gr.cost_initial = res.cost_initial; gr.cost_final = res.cost_final; gr.lambda = res.lambda;
    _bundle = g;
    if (res.status == YGZ_GBA_FAILED) {
        LOG(ERROR) << "LoopClosing::GlobalBundleAdjustment: a map point is not in front of one of its keyframes" << endl;
        return false;
    }

    // 6. the free poses and the included points
    for (int v = 0; v < N; ++v)
        if (!g.fixed[v]) kfs[v]->_TCW = SE3::from7(&g.poses_out[(size_t)v * 7]);
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < 3; ++k) pts[l]->_pos_world[k] = g.points_out[(size_t)l * 3 + k];
    return true;
}

}  // namespace ygz
