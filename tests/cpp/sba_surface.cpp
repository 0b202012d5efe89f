// ygz::BundleAdjuster (include/ygz/Algorithm/BundleAdjuster.h), a stand-alone program for tests/test_sba_surface_build.py and
// tests/test_gpu_sba_surface.py: written against include/ygz only.
//   sba_surface run <dir> <keyframe> <cov,cov,...>
// reads a synthetic stereo map: kf_poses.bin (float64 [K][7]), points.bin and points_behind.bin (float64 [P][3]; the second with one point
// behind one of its keyframes), and the observations in point order: ob_kf.bin, ob_point.bin, ob_level.bin (int32 [M]), ob_px.bin (float64
// [M][3]: u, v, uR), ob_kind.bin (uint8 [M]: 2 gives the keyframe's u_right an entry, 1 leaves -1).  Keyframe k gets one feature per
// observation of it, in file order; keyframe <keyframe> gets the listed covisible keyframes.  The baseline is 0.1 m, the pyramid has 4
// levels, the camera is fx = fy = 500, cx = 320, cy = 240 (camera.bin has what the program used).  Five scenarios, each on a fresh copy of the map:
//   local    LocalBundleAdjustment(<keyframe>) with the defaults         noerase  the same with _erase_outliers = false
//   global   GlobalBundleAdjustment(all keyframes)                       failed   local on points_behind.bin
//   mono     local without any SetURight
// Written to <dir> per scenario <s>: <s>_ret (int32: return value, GetOutlierCount, rounds_run, points_left_out), the problem <s>_kf_ids,
// <s>_point_ids (int64), <s>_poses, <s>_points, <s>_obs, <s>_fixed, <s>_kind, <s>_edge_pose, <s>_edge_point, <s>_level, <s>_edge_feature,
// <s>_poses_out, <s>_points_out, <s>_outlier, <s>_chi2, <s>_status (int32 [4]), <s>_inliers (int32 [4]); the map afterwards <s>_map_poses
// ([K][7]), <s>_map_points ([P][3]), <s>_map_feat (int64 per feature, keyframes in order: the map point's id or -1), <s>_map_obs (int64
// [..][3]: point id, keyframe id, feature index, per point in key order), <s>_map_rest (bytes: everything else of the map); and the map
// before as before_* (before_behind_* for `failed`).  For local and global also the C call on the exported problem: <s>_abi_poses_out,
// <s>_abi_points_out, <s>_abi_outlier, <s>_abi_chi2, <s>_abi_status.
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

struct Files {
    std::vector<double> kf_poses, points, points_behind, px;
    std::vector<int32_t> ob_kf, ob_point, ob_level;
    std::vector<uint8_t> ob_kind;
};

struct World {
    std::vector<Frame *> kfs;
    std::vector<MapPoint *> mps;
    std::vector<std::vector<double>> u_right;
    ~World() { for (Frame *k : kfs) delete k; for (MapPoint *m : mps) delete m; }
};

static void build(World &w, const Files &in, bool behind, int keyframe, const std::vector<int> &cov)
{
    Memory::Clean();
    const size_t K = in.kf_poses.size() / 7, P = in.points.size() / 3;
    const std::vector<double> &X = behind ? in.points_behind : in.points;
    for (size_t k = 0; k < K; ++k) {
        Frame *kf = new Frame;
        Memory::RegisterKeyFrame(kf);
        kf->_id = kf->_keyframe_id;
        kf->_TCW = SE3::from7(&in.kf_poses[7 * k]);
        w.kfs.push_back(kf);
    }
    w.u_right.assign(K, std::vector<double>());
    for (size_t l = 0; l < P; ++l) {
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_pos_world = Vector3d(X[3 * l], X[3 * l + 1], X[3 * l + 2]);
        w.mps.push_back(mp);
    }
    for (size_t i = 0; i < in.ob_kf.size(); ++i) {
        Frame *kf = w.kfs[in.ob_kf[i]];
        MapPoint *mp = w.mps[in.ob_point[i]];
        Feature *f = new Feature(Vector2d(in.px[3 * i], in.px[3 * i + 1]), in.ob_level[i]);
        f->_frame = kf; f->_mappoint = mp;
        kf->_features.push_back(f);
        mp->_obs[kf->_keyframe_id] = f;
        w.u_right[in.ob_kf[i]].push_back(in.ob_kind[i] == 2 ? in.px[3 * i + 2] : -1.0);
    }
    for (int c : cov) { w.kfs[keyframe]->_cov_keyframes.push_back(w.kfs[c]); w.kfs[keyframe]->_cov_weights.push_back(100); }
}

template <typename T> static void push(std::vector<uint8_t> &b, const T &v) { const uint8_t *p = (const uint8_t *)&v; b.insert(b.end(), p, p + sizeof(T)); }

static bool dump_map(const std::string &s, const World &w)
{
    std::vector<double> poses, points;
    std::vector<int64_t> feat, obs;
    std::vector<uint8_t> rest;
    for (const Frame *kf : w.kfs) {
        double t[7]; kf->_TCW.to7(t);
        poses.insert(poses.end(), t, t + 7);
        push(rest, (int64_t)kf->_keyframe_id); push(rest, (int32_t)kf->_bad); push(rest, (int64_t)kf->_features.size());
        for (const Feature *f : kf->_features) {
            feat.push_back(f->_mappoint ? (int64_t)f->_mappoint->_id : -1);
            push(rest, f->_pixel[0]); push(rest, f->_pixel[1]); push(rest, (int32_t)f->_level); push(rest, (int32_t)f->_bad); push(rest, f->_depth);
        }
        push(rest, (int64_t)kf->_cov_keyframes.size());
        for (const Frame *k : kf->_cov_keyframes) push(rest, (int64_t)k->_keyframe_id);
        for (int c : kf->_cov_weights) push(rest, (int32_t)c);
        push(rest, (int64_t)kf->_connected_keyframe_weights.size());
    }
    for (const MapPoint *mp : w.mps) {
        for (int k = 0; k < 3; ++k) points.push_back(mp->_pos_world[k]);
        push(rest, (int64_t)mp->_id); push(rest, (int32_t)mp->_bad); push(rest, (int32_t)mp->_cnt_found); push(rest, (int32_t)mp->_cnt_visible);
        for (const auto &ob : mp->_obs) {
            const Frame *kf = ob.second->_frame;
            int64_t ix = -1;
            for (size_t i = 0; i < kf->_features.size(); ++i) if (kf->_features[i] == ob.second) ix = (int64_t)i;
            obs.push_back((int64_t)mp->_id); obs.push_back((int64_t)ob.first); obs.push_back(ix);
        }
    }
    return put(s + "_poses", poses) && put(s + "_points", points) && put(s + "_feat", feat) && put(s + "_obs", obs) && put(s + "_rest", rest);
}

static bool dump_problem(const std::string &s, const BundleAdjuster &ba, bool ret)
{
    const BundleAdjuster::Problem &g = ba.GetProblem();
    const BundleAdjuster::Result &r = ba.GetResult();
    std::vector<int32_t> status, inliers;
    for (int k = 0; k < 4; ++k) { status.push_back(r._rounds[k]._status); inliers.push_back(r._rounds[k]._inliers); }
    const std::vector<int32_t> rets = { ret ? 1 : 0, ba.GetOutlierCount(), r._rounds_run, g.points_left_out };
    return put(s + "_ret", rets) && put(s + "_kf_ids", std::vector<int64_t>(g.keyframe_ids.begin(), g.keyframe_ids.end())) &&
           put(s + "_point_ids", std::vector<int64_t>(g.point_ids.begin(), g.point_ids.end())) && put(s + "_poses", g.poses) &&
           put(s + "_points", g.points) && put(s + "_obs", g.obs) && put(s + "_fixed", g.fixed) && put(s + "_kind", g.kind) &&
           put(s + "_edge_pose", g.edge_pose) && put(s + "_edge_point", g.edge_point) && put(s + "_level", g.level) &&
           put(s + "_edge_feature", g.edge_feature) && put(s + "_poses_out", g.poses_out) && put(s + "_points_out", g.points_out) &&
           put(s + "_outlier", g.outlier) && put(s + "_chi2", g.chi2) && put(s + "_status", status) && put(s + "_inliers", inliers);
}

// the C call on the problem the class exported
static bool abi_call(const std::string &s, const BundleAdjuster &ba, int rounds, const int *iterations)
{
    const BundleAdjuster::Problem &g = ba.GetProblem();
    const int N = (int)g.fixed.size(), L = (int)g.points.size() / 3, E = (int)g.kind.size();
    ygz_sba_params p;
    ygz_hip_default_sba_params(&p);
    p.baseline = ba._options._baseline; p.rounds = rounds; p.robust_rounds = 1;
    for (int k = 0; k < 4; ++k) p.iterations[k] = k < rounds ? iterations[k] : 0;
    ygz_sba_result res;
    std::vector<double> po((size_t)N * 7), xo((size_t)L * 3), chi2((size_t)E);
    std::vector<uint8_t> outlier((size_t)E);
    if (ygz_hip_stereo_ba(hip::Runtime::Get().ctx(), N, g.poses.data(), g.fixed.data(), L, g.points.data(), E, g.edge_pose.data(), g.edge_point.data(),
                          g.obs.data(), g.kind.data(), g.level.data(), g.K4, &p, po.data(), xo.data(), outlier.data(), chi2.data(), &res) != YGZ_OK)
        return false;
    const std::vector<int32_t> status(res.status, res.status + 4);
    return put(s + "_abi_poses_out", po) && put(s + "_abi_points_out", xo) && put(s + "_abi_outlier", outlier) && put(s + "_abi_chi2", chi2) &&
           put(s + "_abi_status", status);
}

static int run(int keyframe, const std::vector<int> &cov)
{
    Config::Set("image.width", "640"); Config::Set("image.height", "480"); Config::Set("frame.pyramid", "4");
    Config::Set("camera.fx", "500"); Config::Set("camera.fy", "500"); Config::Set("camera.cx", "320"); Config::Set("camera.cy", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Files in;
    if (!get("kf_poses", in.kf_poses) || !get("points", in.points) || !get("points_behind", in.points_behind) || !get("ob_kf", in.ob_kf) ||
        !get("ob_point", in.ob_point) || !get("ob_level", in.ob_level) || !get("ob_px", in.px) || !get("ob_kind", in.ob_kind))
        return 10;
    const std::vector<double> k4 = { (double)cam.fx(), (double)cam.fy(), (double)cam.cx(), (double)cam.cy() };
    if (!put("camera", k4)) return 10;
    const char *names[5] = { "local", "noerase", "global", "failed", "mono" };
    for (int q = 0; q < 5; ++q) {
        const std::string s = names[q];
        World w;
        build(w, in, q == 3, keyframe, cov);
        if (q == 0 && !dump_map("before", w)) return 11;
        if (q == 3 && !dump_map("before_behind", w)) return 11;
        BundleAdjuster ba;                                           // the defaults: baseline 0.1, two rounds of 5 and 10
        if (ba.LocalBundleAdjustment(nullptr) || ba.GlobalBundleAdjustment({})) return 12;
        if (q != 4) for (size_t k = 0; k < w.kfs.size(); ++k) ba.SetURight(w.kfs[k], w.u_right[k]);
        if (q == 1) ba._options._erase_outliers = false;
        const bool ret = q == 2 ? ba.GlobalBundleAdjustment(w.kfs) : ba.LocalBundleAdjustment(w.kfs[keyframe]);
        if (!dump_problem(s, ba, ret) || !dump_map(s + "_map", w)) return 13;
        const int gba_it[4] = { ba._options._gba_iterations, 0, 0, 0 };
        if (q == 0 && !abi_call(s, ba, ba._options._rounds, ba._options._iterations)) return 14;
        if (q == 2 && !abi_call(s, ba, 1, gba_it)) return 14;
    }
    Memory::Clean();
    return 0;
}

int main(int argc, char **argv)
{
    if (!(argc == 5 && !strcmp(argv[1], "run"))) { fprintf(stderr, "usage: sba_surface run <dir> <keyframe> <cov,cov,...>\n"); return 2; }
    g_dir = argv[2];
    std::vector<int> cov;
    for (char *t = strtok(argv[4], ","); t; t = strtok(nullptr, ",")) cov.push_back(atoi(t));
    int rc = 3;
    try {
        rc = run(atoi(argv[3]), cov);
    } catch (const std::exception &ex) {
        fprintf(stderr, "sba_surface: %s\n", ex.what());
        return 4;
    }
    printf("sba_surface: %d\n", rc);
    return rc;
}
