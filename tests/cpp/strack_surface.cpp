// ygz::StereoTracker (include/ygz/Algorithm/StereoTracker.h), a stand-alone program for tests/test_strack_surface_build.py and
// tests/test_gpu_strack_surface.py: written against include/ygz only.
//   strack_surface run <dir>
// reads a synthetic stereo map: kf_poses.bin (float64 [K][7]), kf_bad.bin (uint8 [K]), kf_cov.bin (int32: per keyframe a count and that many
// covisible keyframe indices, in list order), the features in file order: ft_kf (int32 [M]: the keyframe's index; K: the last frame, K + 1:
// the current frame), ft_level, ft_mp (int32 [M]: the map point's index or -1), ft_px (float64 [M][2]), ft_angle, ft_ur (float64 [M]),
// ft_desc (uint8 [M][32]); the map points mp_pos (float64 [P][3]), mp_bad (uint8 [P]); velocity.bin (float64 [7]); last_pose.bin (float64
// [7]).  The baseline is 0.1 m, the pyramid has 4 levels, the camera is fx = fy = 500, cx = 320, cy = 240.  Scenarios, each on a fresh copy:
//   run    TrackWithMotionModel, LocalKeyFrames, TrackLocalMap on a tracker that was given the current frame's right columns
//   mono   TrackWithMotionModel on a tracker without right columns
//   few    TrackWithMotionModel with _min_matches_motion above the number of points: the retry, then 0
// Written to <dir>: mp_ids (int64 [P]); per stage <s> in m (after the motion model), l (after the local map), mono, few: <s>_ret (int32: the
// return value, then the Stats fields in order), <s>_feat (int64 per feature of the current frame: the map point's id or -1), <s>_bad (uint8
// per feature), <s>_pose (float64 [7]), <s>_mp (int64 [P][4]: _cnt_visible, _cnt_found, _track_in_view, _last_seen); per search <q> in s0, s1,
// mono_s0, few_s0: <q>_points (int64 ids), <q>_pw, <q>_dmax, <q>_normal, <q>_angle, <q>_proj, <q>_T (float64), <q>_desc, <q>_taken (uint8),
// <q>_level, <q>_match, <q>_dist, <q>_reason, <q>_outcome, <q>_counts (int32), <q>_head (float64: th, direction); lk (int64: the local
// keyframes' ids), lk_ref (int64: the reference keyframe's id or -1).
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
    std::vector<double> kf_poses, px, angle, ur, mp_pos, velocity, last_pose;
    std::vector<int32_t> kf, level, mp, cov;
    std::vector<uint8_t> desc, kf_bad, mp_bad;
};

struct World {
    std::vector<Frame *> kfs;                       // the keyframes, then the last and the current frame
    std::vector<MapPoint *> mps;
    std::vector<std::vector<double>> u_right;
    Frame *last = nullptr, *current = nullptr;
    ~World() { for (Frame *k : kfs) delete k; }
};

static void build(World &w, const Files &in)
{
    Memory::Clean();
    const size_t K = in.kf_poses.size() / 7;
    for (size_t k = 0; k < K + 2; ++k) {
        Frame *f = new Frame;
        if (k < K) {
            Memory::RegisterKeyFrame(f);
            f->_id = f->_keyframe_id;
            f->_is_keyframe = true;
            f->_TCW = SE3::from7(&in.kf_poses[7 * k]);
            f->_bad = in.kf_bad[k] != 0;
        } else f->_id = 1000 + k;
        w.kfs.push_back(f);
    }
    w.last = w.kfs[K]; w.current = w.kfs[K + 1];
    w.last->_TCW = SE3::from7(in.last_pose.data());
    for (size_t p = 0; p < in.mp_bad.size(); ++p) {
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_pos_world = Vector3d(in.mp_pos[3 * p], in.mp_pos[3 * p + 1], in.mp_pos[3 * p + 2]);
        mp->_bad = in.mp_bad[p] != 0;
        mp->_cnt_visible = mp->_cnt_found = 1;
        w.mps.push_back(mp);
    }
    w.u_right.assign(K + 2, std::vector<double>());
    for (size_t i = 0; i < in.kf.size(); ++i) {
        Frame *fr = w.kfs[in.kf[i]];
        Feature *f = new Feature(Vector2d(in.px[2 * i], in.px[2 * i + 1]), in.level[i]);
        f->_frame = fr; f->_angle = in.angle[i];
        memcpy(f->_desc.data, &in.desc[32 * i], 32);
        if (in.mp[i] >= 0) {
            MapPoint *mp = w.mps[in.mp[i]];
            f->_mappoint = mp;
            if ((size_t)in.kf[i] < K) {                                  // only keyframes observe
                if (mp->_obs.empty()) mp->_first_seen = mp->_last_seen = fr->_keyframe_id;
                mp->_obs[fr->_keyframe_id] = f;
            }
        }
        fr->_features.push_back(f);
        w.u_right[in.kf[i]].push_back(in.ur[i]);
    }
    size_t at = 0;
    for (size_t k = 0; k < K && at < in.cov.size(); ++k) {
        const int n = in.cov[at++];
        for (int j = 0; j < n; ++j) { w.kfs[k]->_cov_keyframes.push_back(w.kfs[in.cov[at++]]); w.kfs[k]->_cov_weights.push_back(100 - j); }
    }
}

static std::vector<int64_t> ids_of(const std::vector<MapPoint *> &v)
{
    std::vector<int64_t> o;
    for (const MapPoint *m : v) o.push_back((int64_t)m->_id);
    return o;
}

static bool dump_stage(const std::string &s, const World &w, int ret, const StereoTracker::Stats &st)
{
    const std::vector<int32_t> rets = { ret, st.direction, st.retried, st.motion_points, st.motion_matches, st.motion_inliers, st.motion_kept,
                                        st.local_keyframes, st.local_on_frame, st.local_points, st.local_cut, st.local_searched, st.local_matches,
                                        st.local_inliers, st.local_kept };
    std::vector<int64_t> feat, mp;
    std::vector<uint8_t> bad;
    for (const Feature *f : w.current->_features) { feat.push_back(f->_mappoint ? (int64_t)f->_mappoint->_id : -1); bad.push_back(f->_bad ? 1 : 0); }
    for (const MapPoint *m : w.mps) {
        mp.push_back(m->_cnt_visible); mp.push_back(m->_cnt_found); mp.push_back(m->_track_in_view ? 1 : 0); mp.push_back((int64_t)m->_last_seen);
    }
    std::vector<double> pose(7);
    w.current->_TCW.to7(pose.data());
    return put(s + "_ret", rets) && put(s + "_feat", feat) && put(s + "_bad", bad) && put(s + "_pose", pose) && put(s + "_mp", mp);
}

static bool dump_search(const std::string &q, const StereoTracker::Search &s)
{
    const std::vector<double> T(s.T, s.T + 7), head = { s.th, (double)s.direction };
    const std::vector<int32_t> counts(s.counts, s.counts + 4);
    return put(q + "_points", ids_of(s.points)) && put(q + "_pw", s.pw) && put(q + "_dmax", s.dmax) && put(q + "_normal", s.normal) &&
           put(q + "_angle", s.angle) && put(q + "_proj", s.proj) && put(q + "_T", T) && put(q + "_desc", s.desc) && put(q + "_taken", s.taken) &&
           put(q + "_level", s.level) && put(q + "_match", s.match) && put(q + "_dist", s.dist) && put(q + "_reason", s.reason) &&
           put(q + "_outcome", s.outcome) && put(q + "_counts", counts) && put(q + "_head", head);
}

static int run()
{
    Config::Set("image.width", "640"); Config::Set("image.height", "480"); Config::Set("frame.pyramid", "4");
    Config::Set("camera.fx", "500"); Config::Set("camera.fy", "500"); Config::Set("camera.cx", "320"); Config::Set("camera.cy", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Files in;
    if (!get("kf_poses", in.kf_poses) || !get("kf_bad", in.kf_bad) || !get("kf_cov", in.cov) || !get("ft_kf", in.kf) || !get("ft_level", in.level) ||
        !get("ft_mp", in.mp) || !get("ft_px", in.px) || !get("ft_angle", in.angle) || !get("ft_ur", in.ur) || !get("ft_desc", in.desc) ||
        !get("mp_pos", in.mp_pos) || !get("mp_bad", in.mp_bad) || !get("velocity", in.velocity) || !get("last_pose", in.last_pose) ||
        in.velocity.size() != 7 || in.last_pose.size() != 7)
        return 10;
    const SE3 velocity = SE3::from7(in.velocity.data());
    const size_t K = in.kf_poses.size() / 7;
    {   // run
        World w;
        build(w, in);
        if (!put("mp_ids", ids_of(w.mps))) return 11;
        StereoTracker tr;
        PoseOptimizer opt;
        if (tr.TrackWithMotionModel(nullptr, w.last, velocity, opt) != 0 || tr.LocalKeyFrames(nullptr, nullptr) != 0) return 12;
        tr.SetURight(w.current, w.u_right[K + 1]);
        tr.SetURight(w.last, w.u_right[K]);
        tr.ClearURight(w.last);
        const int r0 = tr.TrackWithMotionModel(w.current, w.last, velocity, opt);
        if (!dump_stage("m", w, r0, tr.GetStats()) || !dump_search("s0", tr.GetSearch(0))) return 13;
        std::vector<Frame *> local;
        const int nl = tr.LocalKeyFrames(w.current, &local);
        std::vector<int64_t> lk, ref(1, w.current->_ref_keyframe ? (int64_t)w.current->_ref_keyframe->_keyframe_id : -1);
        for (const Frame *f : local) lk.push_back((int64_t)f->_keyframe_id);
        if (nl != (int)local.size() || !put("lk", lk) || !put("lk_ref", ref)) return 14;
        const int r1 = tr.TrackLocalMap(w.current, local, opt);
        if (!dump_stage("l", w, r1, tr.GetStats()) || !dump_search("s1", tr.GetSearch(1))) return 15;
    }
    {   // mono
        World w;
        build(w, in);
        StereoTracker tr;
        PoseOptimizer opt;
        const int r = tr.TrackWithMotionModel(w.current, w.last, velocity, opt);
        if (!dump_stage("mono", w, r, tr.GetStats()) || !dump_search("mono_s0", tr.GetSearch(0))) return 16;
    }
    {   // few
        World w;
        build(w, in);
        StereoTracker tr;
        PoseOptimizer opt;
        tr._options._min_matches_motion = 1000000;
        tr.SetURight(w.current, w.u_right[K + 1]);
        const int r = tr.TrackWithMotionModel(w.current, w.last, velocity, opt);
        if (!dump_stage("few", w, r, tr.GetStats()) || !dump_search("few_s0", tr.GetSearch(0))) return 17;
    }
    Memory::Clean();
    return 0;
}

int main(int argc, char **argv)
{
    if (!(argc == 3 && !strcmp(argv[1], "run"))) { fprintf(stderr, "usage: strack_surface run <dir>\n"); return 2; }
    g_dir = argv[2];
    int rc = 3;
    try {
        rc = run();
    } catch (const std::exception &ex) {
        fprintf(stderr, "strack_surface: %s\n", ex.what());
        return 4;
    }
    printf("strack_surface: %s\n", rc == 0 ? "ok" : "failed");
    return rc;
}
