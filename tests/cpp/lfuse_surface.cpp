// ygz::StereoMapper::SearchInNeighbors / MapPointCulling (include/ygz/Algorithm/StereoMapper.h), a stand-alone program for
// tests/test_lfuse_surface_build.py and tests/test_gpu_lfuse_surface.py: written against include/ygz only.
//   lfuse_surface run <dir> <keyframe> <cull keyframe>
// reads a synthetic stereo map: kf_poses.bin (float64 [K][7]), kf_bad.bin (uint8 [K]), kf_cov.bin (int32: per keyframe a count and that many
// covisible keyframe indices, in list order), the features in file order: ft_kf, ft_level, ft_node, ft_mp (int32 [M]: the map point's index
// or -1), ft_px (float64 [M][2]), ft_depth, ft_ur (float64 [M]), ft_desc (uint8 [M][32]); the map points mp_pos (float64 [P][3]), mp_bad
// (uint8 [P]); cull_edit.bin (int32 [..][4]: bad, _cnt_found, _cnt_visible, _first_seen for the first points of the recent list).  The
// baseline is 0.1 m, the pyramid has 4 levels, the camera is fx = fy = 500, cx = 320, cy = 240.  Scenarios, each on a fresh copy of the map:
//   sin    SearchInNeighbors(<keyframe>), then LoopClosing::UpdateCovisibility(GetTouched(), all) and BundleAdjuster::LocalBundleAdjustment
//   bad    SearchInNeighbors with _fuse_chi2_mono = -1: the device call is refused
//   cull   CreateNewMapPoints and CreateKeyframePoints of <keyframe> (the recent list in creation order), the edits, MapPointCulling(<cull
//          keyframe>) with _cull_min_obs = 1 on a mapper that was given no right columns, ClearRecent
// Written to <dir>: mp_ids (int64 [P]: the ids the map points got); per scenario <s> the map afterwards: <s>_feat (int64 per feature in
// keyframe order, then feature order: the map point's id or -1), <s>_mp (int64 [..][6]: id, _first_seen, _last_seen, _cnt_visible,
// _cnt_found, _bad), <s>_mp_obs (int64 [..][3]: point id, keyframe id, feature index), <s>_mp_dd (uint8: the point has a distinctive
// descriptor); the map before as before_*.  sin_ret (int32: the return value and the FuseStats fields in order), sin_fusions (int64 [..][5]),
// sin_touched, sin_targets (int64 ids), per direction r = 0, 1: s<r>_points (int64 ids), s<r>_pw, s<r>_dmax, s<r>_normal (float64), s<r>_desc,
// s<r>_skip (uint8), s<r>_match (int32); sin_cov (int64 [..][2]: the keyframe's _cov_keyframes ids and weights after UpdateCovisibility),
// sin_conn (int64 [..][2]: its _connected_keyframe_weights by id), sin_ba (int32: LocalBundleAdjustment's return value, points, edges);
// bad_ret (int32: return value, fusions, targets); cull_ret (int32: created by CreateNewMapPoints, by CreateKeyframePoints, culled, the
// list's length after, after ClearRecent), cull_recent, cull_created, cull_after (int64 ids).
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
    std::vector<double> kf_poses, px, depth, ur, mp_pos;
    std::vector<int32_t> kf, level, node, mp, cov, edit;
    std::vector<uint8_t> desc, kf_bad, mp_bad;
};

struct World {
    std::vector<Frame *> kfs;
    std::vector<MapPoint *> mps;
    std::vector<std::vector<double>> u_right;
    ~World() { for (Frame *k : kfs) delete k; }
};

static void build(World &w, const Files &in)
{
    Memory::Clean();
    const size_t K = in.kf_poses.size() / 7;
    for (size_t k = 0; k < K; ++k) {
        Frame *kf = new Frame;
        Memory::RegisterKeyFrame(kf);
        kf->_id = kf->_keyframe_id;
        kf->_TCW = SE3::from7(&in.kf_poses[7 * k]);
        kf->_bad = in.kf_bad[k] != 0;
        w.kfs.push_back(kf);
    }
    for (size_t p = 0; p < in.mp_bad.size(); ++p) {
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_pos_world = Vector3d(in.mp_pos[3 * p], in.mp_pos[3 * p + 1], in.mp_pos[3 * p + 2]);
        mp->_bad = in.mp_bad[p] != 0;
        mp->_cnt_visible = mp->_cnt_found = 1;
        w.mps.push_back(mp);
    }
    w.u_right.assign(K, std::vector<double>());
    for (size_t i = 0; i < in.kf.size(); ++i) {
        Frame *kf = w.kfs[in.kf[i]];
        Feature *f = new Feature(Vector2d(in.px[2 * i], in.px[2 * i + 1]), in.level[i]);
        f->_frame = kf; f->_depth = in.depth[i];
        memcpy(f->_desc.data, &in.desc[32 * i], 32);
        if (in.node[i] >= 0) kf->_feature_vec[(unsigned int)in.node[i]].push_back((unsigned int)kf->_features.size());
        if (in.mp[i] >= 0) {
            MapPoint *mp = w.mps[in.mp[i]];
            if (mp->_obs.empty()) mp->_first_seen = mp->_last_seen = kf->_keyframe_id;
            mp->_obs[kf->_keyframe_id] = f;
            f->_mappoint = mp;
        }
        kf->_features.push_back(f);
        w.u_right[in.kf[i]].push_back(in.ur[i]);
    }
    size_t at = 0;
    for (size_t k = 0; k < K && at < in.cov.size(); ++k) {
        const int n = in.cov[at++];
        for (int j = 0; j < n; ++j) { w.kfs[k]->_cov_keyframes.push_back(w.kfs[in.cov[at++]]); w.kfs[k]->_cov_weights.push_back(100 - j); }
    }
}

static bool dump_map(const std::string &s, const World &w, const std::vector<MapPoint *> &created)
{
    std::vector<int64_t> feat, mp, obs;
    std::vector<uint8_t> dd;
    for (const Frame *kf : w.kfs)
        for (const Feature *f : kf->_features) feat.push_back(f->_mappoint ? (int64_t)f->_mappoint->_id : -1);
    std::vector<MapPoint *> all = w.mps;
    all.insert(all.end(), created.begin(), created.end());
    for (const MapPoint *m : all) {
        mp.push_back((int64_t)m->_id); mp.push_back((int64_t)m->_first_seen); mp.push_back((int64_t)m->_last_seen);
        mp.push_back(m->_cnt_visible); mp.push_back(m->_cnt_found); mp.push_back(m->_bad ? 1 : 0);
        dd.push_back(m->_distinctive_desc.data && m->_distinctive_desc.rows * m->_distinctive_desc.cols == 32 ? 1 : 0);
        for (const auto &ob : m->_obs) {
            const Frame *kf = ob.second->_frame;
            int64_t ix = -1;
            for (size_t i = 0; i < kf->_features.size(); ++i) if (kf->_features[i] == ob.second) ix = (int64_t)i;
            obs.push_back((int64_t)m->_id); obs.push_back((int64_t)ob.first); obs.push_back(ix);
        }
    }
    return put(s + "_feat", feat) && put(s + "_mp", mp) && put(s + "_mp_obs", obs) && put(s + "_mp_dd", dd);
}

static std::vector<int64_t> ids_of(const std::vector<MapPoint *> &v)
{
    std::vector<int64_t> o;
    for (const MapPoint *m : v) o.push_back((int64_t)m->_id);
    return o;
}

static int run(int keyframe, int cull_kf)
{
    Config::Set("image.width", "640"); Config::Set("image.height", "480"); Config::Set("frame.pyramid", "4");
    Config::Set("camera.fx", "500"); Config::Set("camera.fy", "500"); Config::Set("camera.cx", "320"); Config::Set("camera.cy", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Files in;
    if (!get("kf_poses", in.kf_poses) || !get("kf_bad", in.kf_bad) || !get("kf_cov", in.cov) || !get("ft_kf", in.kf) || !get("ft_level", in.level) ||
        !get("ft_node", in.node) || !get("ft_mp", in.mp) || !get("ft_px", in.px) || !get("ft_depth", in.depth) || !get("ft_ur", in.ur) ||
        !get("ft_desc", in.desc) || !get("mp_pos", in.mp_pos) || !get("mp_bad", in.mp_bad) || !get("cull_edit", in.edit))
        return 10;
    const std::vector<MapPoint *> none;
    {   // sin
        World w;
        build(w, in);
        if (!put("mp_ids", ids_of(w.mps)) || !dump_map("before", w, none)) return 11;
        StereoMapper sm;
        Matcher matcher;
        if (sm.SearchInNeighbors(nullptr, matcher) != 0) return 12;
        for (size_t k = 0; k < w.kfs.size(); ++k) sm.SetURight(w.kfs[k], w.u_right[k]);
        const int ret = sm.SearchInNeighbors(w.kfs[keyframe], matcher);
        const StereoMapper::FuseStats &st = sm.GetStats();
        const std::vector<int32_t> rets = { ret, st.targets, st.targets_dropped, st.forward_points, st.forward_hits, st.reverse_points, st.reverse_cut,
                                            st.reverse_hits, st.added, st.replaced, st.conflicts, st.descriptors };
        std::vector<int64_t> fus, touched, targets;
        for (const auto &f : sm.GetFusions()) {
            fus.push_back(f.kind); fus.push_back((int64_t)f.target); fus.push_back((int64_t)f.point); fus.push_back(f.feature); fus.push_back((int64_t)f.survivor);
        }
        for (const Frame *f : sm.GetTouched()) touched.push_back((int64_t)f->_keyframe_id);
        for (const Frame *f : sm.GetTargets()) targets.push_back((int64_t)f->_keyframe_id);
        if (!put("sin_ret", rets) || !put("sin_fusions", fus) || !put("sin_touched", touched) || !put("sin_targets", targets) || !dump_map("sin", w, none))
            return 13;
        for (int r = 0; r < 2; ++r) {
            const StereoMapper::Search &s = sm.GetSearch(r);
            const std::string p = r ? "s1" : "s0";
            if (!put(p + "_points", ids_of(s.points)) || !put(p + "_pw", s.pw) || !put(p + "_dmax", s.dmax) || !put(p + "_normal", s.normal) ||
                !put(p + "_desc", s.desc) || !put(p + "_skip", s.skip) || !put(p + "_match", s.match))
                return 14;
        }
        LoopClosing lc;
        lc.UpdateCovisibility(sm.GetTouched(), w.kfs);
        std::vector<int64_t> cov, conn;
        const Frame *cur = w.kfs[keyframe];
        for (size_t i = 0; i < cur->_cov_keyframes.size(); ++i) { cov.push_back((int64_t)cur->_cov_keyframes[i]->_keyframe_id); cov.push_back(cur->_cov_weights[i]); }
        std::map<unsigned long, int> by_id;
        for (const auto &c : cur->_connected_keyframe_weights) by_id[c.first->_keyframe_id] = c.second;
        for (const auto &c : by_id) { conn.push_back((int64_t)c.first); conn.push_back(c.second); }
        BundleAdjuster ba;
        for (size_t k = 0; k < w.kfs.size(); ++k) ba.SetURight(w.kfs[k], w.u_right[k]);
        const bool ok = ba.LocalBundleAdjustment(w.kfs[keyframe]);
        const std::vector<int32_t> bar = { ok ? 1 : 0, (int32_t)ba.GetProblem().point_ids.size(), (int32_t)ba.GetProblem().edge_pose.size() };
        if (!put("sin_cov", cov) || !put("sin_conn", conn) || !put("sin_ba", bar)) return 15;
    }
    {   // bad
        World w;
        build(w, in);
        StereoMapper sm;
        Matcher matcher;
        for (size_t k = 0; k < w.kfs.size(); ++k) sm.SetURight(w.kfs[k], w.u_right[k]);
        sm._options._fuse_chi2_mono = -1.0;
        const int ret = sm.SearchInNeighbors(w.kfs[keyframe], matcher);
        const std::vector<int32_t> rets = { ret, (int32_t)sm.GetFusions().size(), (int32_t)sm.GetTargets().size() };
        if (!put("bad_ret", rets) || !dump_map("bad", w, none)) return 16;
    }
    {   // cull
        World w;
        build(w, in);
        StereoMapper sm;                                 // no right columns: every observation counts 1
        sm._options._cull_min_obs = 1;
        std::vector<MapPoint *> created;
        const int n1 = sm.CreateNewMapPoints(w.kfs[keyframe]);
        created = sm.GetCreated();
        const int n2 = sm.CreateKeyframePoints(w.kfs[keyframe]);
        created.insert(created.end(), sm.GetCreated().begin(), sm.GetCreated().end());
        const std::vector<MapPoint *> recent = sm.GetRecent();
        for (size_t i = 0; i < recent.size() && 4 * i + 3 < in.edit.size(); ++i) {
            MapPoint *p = recent[i];
            p->_bad = in.edit[4 * i] != 0; p->_cnt_found = in.edit[4 * i + 1]; p->_cnt_visible = in.edit[4 * i + 2];
            p->_first_seen = (unsigned long)in.edit[4 * i + 3];
        }
        if (!dump_map("edited", w, created)) return 17;
        const int culled = sm.MapPointCulling(w.kfs[cull_kf]);
        const std::vector<MapPoint *> after = sm.GetRecent();
        sm.ClearRecent();
        const std::vector<int32_t> rets = { n1, n2, culled, (int32_t)after.size(), (int32_t)sm.GetRecent().size() };
        if (!put("cull_ret", rets) || !put("cull_recent", ids_of(recent)) || !put("cull_created", ids_of(created)) || !put("cull_after", ids_of(after)) ||
            !dump_map("cull", w, created))
            return 18;
    }
    Memory::Clean();
    return 0;
}

int main(int argc, char **argv)
{
    if (!(argc == 5 && !strcmp(argv[1], "run"))) { fprintf(stderr, "usage: lfuse_surface run <dir> <keyframe> <cull keyframe>\n"); return 2; }
    g_dir = argv[2];
    int rc = 3;
    try {
        rc = run(atoi(argv[3]), atoi(argv[4]));
    } catch (const std::exception &ex) {
        fprintf(stderr, "lfuse_surface: %s\n", ex.what());
        return 4;
    }
    printf("lfuse_surface: %s\n", rc == 0 ? "ok" : "failed");
    return rc;
}
