// ygz::LoopClosing::CorrectLoop (include/ygz/Algorithm/LoopClosing.h): nothing in the reference, whose loop closing is empty.  The correcting
// half of ORB-SLAM2's LoopClosing::CorrectLoop with Optimizer::OptimizeEssentialGraph's graph: the accepted Sim3 propagated to the current
// keyframe's neighbourhood, one ygz_hip_pose_graph_optimize call (ygz_slam_amd/csrc/pgo.hip), poses and map points rewritten from its result.
// Every choice ORB-SLAM2 leaves to set iteration over pointers goes by keyframe id here.  Fusion and the covisibility update are FuseLoop
// (ygz_fuse.cpp), the global BA GlobalBundleAdjustment (ygz_gba.cpp).
// Error conventions of the other surfaces: a failed call logs and returns false, only a missing device throws.
#include "ygz/Algorithm/LoopClosing.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <algorithm>

namespace ygz {

namespace {
bool by_id(const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; }

// (R, t / s) of S: the camera pose in the units of the corrected world
SE3 pose_of(const Sim3 &S) { return SE3(S.R, S.t / S.s); }
}

bool LoopClosing::CorrectLoop()
{
    vector<Frame *> kfs;
    const int n = Memory::GetNumberFrames();
    for (int id = 0; id < n; ++id) {
        Frame *k = Memory::GetKeyFrame((unsigned long)id);
        if (k) kfs.push_back(k);
    }
    return CorrectLoop(kfs);
}

bool LoopClosing::CorrectLoop(const vector<Frame *> &keyframes)
{
    if (!_correctable || !_current || !_matched) return false;
    Stats::PoseGraphResult none;
    _stats.correct_vertices = _stats.correct_tree_edges = _stats.correct_covisibility_edges = _stats.correct_loop_edges = 0;
    _stats.correct_points_moved = 0;
    _stats.correct_left_out.clear();
    _stats.pose_graph = none;

    // 1. the candidates: not bad, once each, by id; the loop's two keyframes have to be among them
    vector<Frame *> cand;
    for (Frame *k : keyframes) if (k && !k->_bad) cand.push_back(k);
    std::sort(cand.begin(), cand.end(), by_id);
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    map<const Frame *, int> index;
    for (size_t i = 0; i < cand.size(); ++i) index[cand[i]] = (int)i;
    if (!index.count(_current) || !index.count(_matched) || _current == _matched) {
        LOG(ERROR) << "LoopClosing::CorrectLoop: the loop's keyframes are not among the keyframes given" << endl;
        return false;
    }
    const int nc = (int)cand.size();

    // the connections among the candidates, symmetric: the larger of the two weights the keyframes hold for each other
    vector<map<int, int>> weight(nc);
    for (int i = 0; i < nc; ++i)
        for (const auto &c : cand[i]->_connected_keyframe_weights) {
            auto it = index.find(c.first);
            if (it == index.end() || it->second == i) continue;
            const int j = it->second;
            weight[i][j] = std::max(weight[i].count(j) ? weight[i][j] : c.second, c.second);
            weight[j][i] = weight[i][j];
        }

    // 3. edges over candidate indices: tree, covisibility, loop
    vector<pair<int, int>> edges;
    std::set<pair<int, int>> joined;
    int n_tree = 0, n_cov = 0;
    for (int i = 0; i < nc; ++i) {
        int best = -1, bw = 0;
        for (const auto &w : weight[i])                               // ascending index = ascending id: the first of equal weights stays
            if (w.first < i && (best < 0 || w.second > bw)) { best = w.first; bw = w.second; }
        if (best < 0) continue;
        edges.push_back(make_pair(i, best));
        joined.insert(make_pair(best, i));
        ++n_tree;
    }
    for (int i = 0; i < nc; ++i)
        for (const auto &w : weight[i]) {
            if (w.first >= i || w.second < _option._min_essential_weight || joined.count(make_pair(w.first, i))) continue;
            edges.push_back(make_pair(i, w.first));
            joined.insert(make_pair(w.first, i));
            ++n_cov;
        }
    const int ic = index[_current], im = index[_matched];
    edges.push_back(make_pair(ic, im));

    // 1. the vertices: the candidates with an edge
    vector<int> vertex(nc, -1);
    vector<char> used(nc, 0);
    for (const auto &e : edges) used[e.first] = used[e.second] = 1;
    vector<Frame *> kfs;
    for (int i = 0; i < nc; ++i) {
        if (!used[i]) { _stats.correct_left_out.push_back(cand[i]->_keyframe_id); continue; }
        vertex[i] = (int)kfs.size();
        kfs.push_back(cand[i]);
    }
    const int N = (int)kfs.size(), E = (int)edges.size();
    if (N > YGZ_PGO_MAX_VERTICES || E > YGZ_PGO_MAX_EDGES) {
        LOG(ERROR) << "LoopClosing::CorrectLoop: " << N << " keyframes, " << E << " edges: above the pose graph's capacity" << endl;
        return false;
    }

    // 2. the estimate, 3. the measurements from the poses before the correction, 4. the fixed vertex
    PoseGraph g;
    g.S.resize((size_t)N * 8); g.fixed.assign(N, 0); g.edges.resize((size_t)E * 2); g.M.resize((size_t)E * 8);
    const SE3 Twc = _current->_TCW.inverse();
    for (int v = 0; v < N; ++v) {
        Frame *k = kfs[v];
        g.keyframe_ids.push_back(k->_keyframe_id);
        Sim3 S(k->_TCW);
        if (k == _current) S = _Scw;
        else if (k != _matched && weight[ic].count(index[k])) S = Sim3(k->_TCW * Twc) * _Scw;
        S.to8(&g.S[(size_t)v * 8]);
    }
    g.fixed[vertex[im]] = 1;
    for (int e = 0; e < E; ++e) {
        const int i = edges[e].first, j = edges[e].second;
        g.edges[2 * e] = vertex[i]; g.edges[2 * e + 1] = vertex[j];
        const Sim3 M = e == E - 1 ? Sim3(_matched->_TCW) * _Scw.inverse() : Sim3(cand[j]->_TCW * cand[i]->_TCW.inverse());
        M.to8(&g.M[(size_t)e * 8]);
    }

    // 5. one solver call
    ygz_pgo_params prm;
    ygz_hip_default_pgo_params(&prm);
    prm.fix_scale = _option._fix_scale ? 1 : 0;
    ygz_pgo_result res;
    g.S_out.resize((size_t)N * 8);
    if (!hip::check(ygz_hip_pose_graph_optimize(hip::Runtime::Get().ctx(), N, g.S.data(), g.fixed.data(), E, g.edges.data(), g.M.data(), &prm,
                                                g.S_out.data(), &res), "pose_graph_optimize"))
        return false;
    _stats.correct_vertices = N; _stats.correct_tree_edges = n_tree; _stats.correct_covisibility_edges = n_cov; _stats.correct_loop_edges = 1;
    Stats::PoseGraphResult &pr = _stats.pose_graph;
    pr.status = res.status; pr.lm_iterations = res.lm_iterations; pr.n_solves = res.n_solves; pr.cg_iterations_total = res.cg_iterations_total;
    pr.cg_capped = res.cg_capped; pr.cost_initial = res.cost_initial; pr.cost_final = res.cost_final; pr.lambda = res.lambda;
    _pose_graph = g;
    if (res.status == YGZ_PGO_FAILED) {
        LOG(ERROR) << "LoopClosing::CorrectLoop: the pose graph's residual is undefined at the initial estimate" << endl;
        return false;
    }

    // 6. poses (the old ones kept for the points), 7. map points
    vector<SE3> old_pose(N);
    vector<Sim3> Sout(N);
    vector<char> changed(N, 0);
    for (int v = 0; v < N; ++v) {
        old_pose[v] = kfs[v]->_TCW;
        Sout[v] = Sim3::from8(&g.S_out[(size_t)v * 8]);
        const Sim3 before(old_pose[v]);
        double a[8], b[8];
        before.to8(a); Sout[v].to8(b);
        changed[v] = memcmp(a, b, sizeof a) != 0;
        if (!g.fixed[v] && changed[v]) kfs[v]->_TCW = pose_of(Sout[v]);
    }
    map<const Frame *, int> vertex_of;
    for (int v = 0; v < N; ++v) vertex_of[kfs[v]] = v;
    std::set<MapPoint *> seen;
    for (int v = 0; v < N; ++v)
        for (Feature *f : kfs[v]->_features) {
            MapPoint *mp = f->_mappoint;
            if (!mp || mp->_bad || !seen.insert(mp).second) continue;
            int r = -1;
            for (const auto &ob : mp->_obs) {                         // key order
                if (!ob.second || !ob.second->_frame) continue;
                auto it = vertex_of.find(ob.second->_frame);
                if (it == vertex_of.end()) continue;
                r = it->second;
                break;
            }
            if (r < 0 || g.fixed[r] || !changed[r]) continue;
            mp->_pos_world = Sout[r].inverse() * (old_pose[r] * mp->_pos_world);
            ++_stats.correct_points_moved;
        }
    _correctable = false;
    _fusable = _searched;                                             // FuseLoop needs the loop map points of before this correction
    _searched = false;
    return true;
}

}  // namespace ygz
