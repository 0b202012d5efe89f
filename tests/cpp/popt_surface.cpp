// ygz::PoseOptimizer (include/ygz/Algorithm/PoseOptimizer.h), a stand-alone program for tests/test_popt_ref.py, tests/test_popt_surface_build.py
// and tests/test_gpu_popt_surface.py: written against include/ygz only.
//   popt_surface uright <dir> <baseline>    no device: reads <dir>/px.bin (float64 [n][2]) and depth.bin (float64 [n]), gives a frame those
//        features and depths, calls PoseOptimizer::URightFromDepth; writes u_right.bin (float64 [n]) and count.bin (the return value and n).
//   popt_surface run <dir>                  reads two frames q = 0, 1 as f<q>_pose.bin (float64 [7]), f<q>_pw.bin, f<q>_obs.bin (float64 [n][3]),
//        f<q>_level.bin (int32 [n]), f<q>_kind.bin (uint8 [n], 1 or 2).  Every edge becomes a feature with a map point; frame 0 gets four more
//        features that are no edges (three without a map point, one whose map point is bad).  The baseline is 0.1 m, the pyramid has 4 levels.
// Written to <dir> by `run`, per feature in feature order unless said otherwise:
//   s<q>_pose, s<q>_bad (uint8), s<q>_depth, s<q>_outlier (GetOutliers), s<q>_found (int32: MapPoint::_cnt_found, -1 without a map point),
//   s<q>_ret (int32: Optimize's return value, GetInliers()[0], the rounds that ran), s<q>_status (int32 per round)   -- Optimize per frame
//   abi<q>_pose, abi<q>_outlier (uint8 per edge), abi<q>_counts (int32: inliers, rounds_run), abi<q>_status (int32 [8])  -- the C call on the arrays
//   b_pose (float64 [2][7]), b_bad (uint8, frame 0's features then frame 1's), b_inliers (int32 [2])               -- OptimizeBatch on fresh copies
//   d_pose, d_count (int32: URightFromDepth's return value, the stereo edges), d_ret  -- frame 0 with depths instead of u_right, URightFromDepth
//   m_pose                                                                         -- frame 0 without u_right: mono edges only
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace ygz;

static std::string g_dir;

template <typename T> static bool get(const std::string &name, std::vector<T> &v)
{
    FILE *f = fopen((g_dir + "/" + name + ".bin").c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    const bool ok = bytes >= 0 && (size_t)bytes % sizeof(T) == 0 && fread(v.data(), 1, (size_t)bytes, f) == (size_t)bytes;
    fclose(f);
    return ok;
}

template <typename T> static bool put(const std::string &name, const std::vector<T> &v)
{
    FILE *f = fopen((g_dir + "/" + name + ".bin").c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

struct Edges { std::vector<double> pose, pw, obs; std::vector<int32_t> level; std::vector<uint8_t> kind; };

static bool read_edges(const std::string &q, Edges &e)
{
    return get("f" + q + "_pose", e.pose) && get("f" + q + "_pw", e.pw) && get("f" + q + "_obs", e.obs) && get("f" + q + "_level", e.level) &&
           get("f" + q + "_kind", e.kind) && e.pose.size() == 7 && e.pw.size() == 3 * e.level.size() && e.obs.size() == e.pw.size() &&
           e.kind.size() == e.level.size();
}

// a frame with one feature per edge (and, with `extra`, four features that are no edges); u_right as StereoMatcher would hand it over
static void build(Frame &f, const Edges &e, bool extra, std::vector<double> &u_right, std::vector<MapPoint *> &mps)
{
    f._TCW = SE3::from7(e.pose.data());
    u_right.clear();
    for (size_t i = 0; i < e.level.size(); ++i) {
        Feature *ft = new Feature(Vector2d(e.obs[3 * i], e.obs[3 * i + 1]), e.level[i]);
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_pos_world = Vector3d(e.pw[3 * i], e.pw[3 * i + 1], e.pw[3 * i + 2]);
        ft->_mappoint = mp; ft->_frame = &f;
        f._features.push_back(ft);
        mps.push_back(mp);
        u_right.push_back(e.kind[i] == 2 ? e.obs[3 * i + 2] : -1.0);
    }
    if (!extra) return;
    for (int k = 0; k < 4; ++k) {
        Feature *ft = new Feature(Vector2d(100.0 + k, 50.0), 0);
        ft->_frame = &f;
        if (k == 3) { MapPoint *mp = Memory::CreateMapPoint(); mp->_pos_world = Vector3d(0, 0, 5); mp->_bad = true; ft->_mappoint = mp; mps.push_back(mp); }
        f._features.push_back(ft);
        u_right.push_back(k == 1 ? 90.0 : -1.0);
    }
}

static std::vector<double> pose_of(const Frame &f) { std::vector<double> p(7); f._TCW.to7(p.data()); return p; }

static bool dump(const std::string &q, const Frame &f, const PoseOptimizer &po, int ret)
{
    std::vector<uint8_t> bad;
    std::vector<double> depth;
    std::vector<int32_t> found, status;
    for (const Feature *ft : f._features) {
        bad.push_back(ft->_bad ? 1 : 0); depth.push_back(ft->_depth);
        found.push_back(ft->_mappoint ? (int32_t)ft->_mappoint->_cnt_found : -1);
    }
    if (po.GetOutliers().size() != 1 || po.GetRounds().size() != 1 || po.GetInliers().size() != 1) return false;
    for (const PoseOptimizer::Round &r : po.GetRounds()[0]) status.push_back(r._status);
    const std::vector<int32_t> rets = { ret, po.GetInliers()[0], (int32_t)po.GetRounds()[0].size() };
    return put("s" + q + "_pose", pose_of(f)) && put("s" + q + "_bad", bad) && put("s" + q + "_depth", depth) && put("s" + q + "_outlier", po.GetOutliers()[0]) &&
           put("s" + q + "_found", found) && put("s" + q + "_ret", rets) && put("s" + q + "_status", status);
}

static int run()
{
    Config::Set("image.width", "640"); Config::Set("image.height", "480"); Config::Set("frame.pyramid", "4");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Edges e[2];
    if (!read_edges("0", e[0]) || !read_edges("1", e[1]) || e[0].level.empty() || e[1].level.empty()) return 10;
    std::vector<MapPoint *> mps;
    PoseOptimizer po;                                            // the defaults: baseline 0.1
    if (po.Optimize(nullptr) != 0) return 11;

    // Optimize per frame, and the C call on the same arrays
    hip::Runtime &rt = hip::Runtime::Get();
    for (int q = 0; q < 2; ++q) {
        Frame f;
        std::vector<double> ur;
        build(f, e[q], q == 0, ur, mps);
        std::vector<double> wrong(ur.size() + 1, -1.0);
        if (po.Optimize(&f, &wrong) != 0 || f._features[0]->_bad) return 12;           // a u_right of another length: refused, nothing touched
        const int ret = po.Optimize(&f, &ur);
        if (!dump(std::to_string(q), f, po, ret)) return 13;

        const int n = (int)e[q].level.size();
        const std::vector<int32_t> off = { 0, n };
        ygz_pose_opt_params p;
        ygz_hip_default_pose_opt_params(&p);
        p.baseline = 0.1;
        std::vector<double> pose = e[q].pose;
        std::vector<uint8_t> outlier((size_t)n);
        std::vector<int32_t> counts(2), status(8);
        if (ygz_hip_optimize_pose_stereo(rt.ctx(), 1, off.data(), e[q].pw.data(), e[q].obs.data(), e[q].level.data(), e[q].kind.data(), &p, pose.data(),
                                         outlier.data(), nullptr, &counts[0], &counts[1], status.data(), nullptr, nullptr, nullptr, nullptr) != YGZ_OK)
            return 14;
        const std::string a = "abi" + std::to_string(q);
        if (!put(a + "_pose", pose) || !put(a + "_outlier", outlier) || !put(a + "_counts", counts) || !put(a + "_status", status)) return 15;
    }

    // OptimizeBatch on fresh copies of both frames
    {
        Frame f0, f1;
        std::vector<double> u0, u1;
        build(f0, e[0], true, u0, mps);
        build(f1, e[1], false, u1, mps);
        po.OptimizeBatch({ &f0, &f1 }, { &u0, &u1 });
        if (po.GetInliers().size() != 2) return 16;
        std::vector<double> poses = pose_of(f0), p1 = pose_of(f1);
        poses.insert(poses.end(), p1.begin(), p1.end());
        std::vector<uint8_t> bad;
        for (const Feature *ft : f0._features) bad.push_back(ft->_bad ? 1 : 0);
        for (const Feature *ft : f1._features) bad.push_back(ft->_bad ? 1 : 0);
        const std::vector<int32_t> inl(po.GetInliers().begin(), po.GetInliers().end());
        if (!put("b_pose", poses) || !put("b_bad", bad) || !put("b_inliers", inl)) return 17;
    }

    // depths instead of u_right: URightFromDepth turns the features with a depth into stereo edges
    {
        Frame f;
        std::vector<double> ur, from_depth;
        build(f, e[0], true, ur, mps);
        const double bf = (double)cam.fx() * 0.1;
        int stereo = 0;
        for (size_t i = 0; i < e[0].level.size(); ++i)
            if (e[0].kind[i] == 2) { f._features[i]->_depth = bf / (e[0].obs[3 * i] - e[0].obs[3 * i + 2]); ++stereo; }
        const int cnt = PoseOptimizer::URightFromDepth(&f, 0.1, &from_depth);
        if (from_depth.size() != f._features.size()) return 18;
        const int ret = po.Optimize(&f, &from_depth);
        const std::vector<int32_t> counts = { cnt, stereo }, rets = { ret };
        if (!put("d_pose", pose_of(f)) || !put("d_count", counts) || !put("d_ret", rets)) return 19;
    }
    {
        Frame f;
        std::vector<double> ur;
        build(f, e[0], true, ur, mps);
        po.Optimize(&f);
        if (!put("m_pose", pose_of(f))) return 20;
    }
    return 0;
}

static int uright(const char *baseline)
{
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    std::vector<double> px, depth, ur;
    if (!get("px", px) || !get("depth", depth) || px.size() != 2 * depth.size()) return 10;
    Frame f;
    for (size_t i = 0; i < depth.size(); ++i) {
        Feature *ft = new Feature(Vector2d(px[2 * i], px[2 * i + 1]), 0);
        ft->_depth = depth[i];
        f._features.push_back(ft);
    }
    const int cnt = PoseOptimizer::URightFromDepth(&f, atof(baseline), &ur);
    if (PoseOptimizer::URightFromDepth(nullptr, 0.1, &ur) != 0 || PoseOptimizer::URightFromDepth(&f, 0.1, nullptr) != 0) return 11;
    const std::vector<int32_t> count = { cnt, (int32_t)depth.size() };
    return put("u_right", ur) && put("count", count) ? 0 : 12;
}

int main(int argc, char **argv)
{
    const bool is_run = argc == 3 && !strcmp(argv[1], "run"), is_ur = argc == 4 && !strcmp(argv[1], "uright");
    if (!is_run && !is_ur) { fprintf(stderr, "usage: popt_surface run <dir> | popt_surface uright <dir> <baseline>\n"); return 2; }
    g_dir = argv[2];
    int rc = 3;
    try {
        rc = is_run ? run() : uright(argv[3]);
    } catch (const std::exception &ex) {
        fprintf(stderr, "popt_surface: %s\n", ex.what());
        return 4;
    }
    printf("popt_surface: %d\n", rc);
    return rc;
}
