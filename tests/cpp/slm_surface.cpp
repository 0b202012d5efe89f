// ygz::StereoLocalMap (include/ygz/Algorithm/StereoLocalMap.h), a stand-alone program for tests/test_slm_surface_build.py and
// tests/test_gpu_slm_surface.py: written against include/ygz only.
//   slm_surface <dir>
// reads a small stereo map: four QVGA gray pictures img0 .. img3 (uint8 [240][320]), per frame k its features f<k>_px (float64 [n][2]),
// f<k>_level (int32 [n]), f<k>_angle, f<k>_depth (float64 [n]; <= 0: none), f<k>_mp (int32 [n]: the map point a motion-model stage left on
// the feature, or -1) and f<k>_pose (float64 [7]); three keyframes kf_poses (float64 [3][7]) with their features in file order kft_kf, kft_level,
// kft_mp (int32 [M]), kft_px (float64 [M][2]), kft_desc (uint8 [M][32]); the map points mp_pos (float64 [P][3]).  Frames 0, 1, 2 are tracked
// against the list (kf 0, kf 1, kf 2), frame 3 against (kf 1, kf 2).  A frame feature's _desc is what the device describes at its pixel, so
// that the host-array route sees the descriptors the resident route computes.  Scenarios, each on a fresh copy of the map:
//   old     per frame in order: StereoTracker::SetURight(PoseOptimizer::URightFromDepth), StereoTracker::TrackLocalMap
//   batch   ONE StereoLocalMap::TrackLocalMap over the four frames
//   single  StereoLocalMap::TrackLocalMap of frame 1 alone
// Written to <dir>: per scenario <s>: <s>_pose (float64 [4][7]), <s>_feat<k> (int32 per feature: the map point's index or -1), <s>_bad<k> (uint8),
// <s>_depth<k> (float64), <s>_mp (int32 [P][3]: _cnt_visible, _cnt_found, _track_in_view), <s>_ret (int32: old: the four return values; batch,
// single: the return value, then per frame status, new_matches, edges, inliers, tracked); untouched (int32: 1 when no scenario made a map
// point or a keyframe).
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace ygz;

static std::string g_dir;
static const int W = 320, H = 240, NF = 4, NK = 3;

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

struct FrameIn { std::vector<uint8_t> img; std::vector<double> px, angle, depth, pose; std::vector<int32_t> level, mp; };
struct Files {
    FrameIn fr[NF];
    std::vector<double> kf_poses, kft_px, mp_pos;
    std::vector<int32_t> kft_kf, kft_level, kft_mp;
    std::vector<uint8_t> kft_desc;
};

static bool read_all(Files &in)
{
    for (int k = 0; k < NF; ++k) {
        FrameIn &f = in.fr[k];
        const std::string s = std::to_string(k);
        if (!get("img" + s, f.img) || f.img.size() != (size_t)W * H || !get("f" + s + "_px", f.px) || !get("f" + s + "_level", f.level) ||
            !get("f" + s + "_angle", f.angle) || !get("f" + s + "_depth", f.depth) || !get("f" + s + "_mp", f.mp) || !get("f" + s + "_pose", f.pose) ||
            f.px.size() != 2 * f.level.size() || f.angle.size() != f.level.size() || f.depth.size() != f.level.size() ||
            f.mp.size() != f.level.size() || f.pose.size() != 7 || f.level.empty())
            return false;
    }
    return get("kf_poses", in.kf_poses) && in.kf_poses.size() == 7 * NK && get("kft_kf", in.kft_kf) && get("kft_level", in.kft_level) &&
           get("kft_mp", in.kft_mp) && get("kft_px", in.kft_px) && get("kft_desc", in.kft_desc) && get("mp_pos", in.mp_pos) &&
           in.kft_px.size() == 2 * in.kft_kf.size() && in.kft_desc.size() == 32 * in.kft_kf.size();
}

struct World {
    std::vector<Frame *> kfs, frames;
    std::vector<MapPoint *> mps;
    std::map<const MapPoint *, int32_t> index;
    std::vector<Frame *> list_a, list_b;
    ~World() { for (Frame *k : kfs) delete k; for (Frame *f : frames) delete f; }
};

// the descriptors the device computes for the frame's features, into Feature::_desc
static bool describe(Frame *f)
{
    hip::Runtime &rt = hip::Runtime::Get();
    const int slot = rt.Resident(f), m = (int)f->_features.size(), cells = rt.cells();
    if (slot < 0 || m > cells) return false;
    std::vector<double> px(2 * (size_t)cells);
    std::vector<int32_t> lvl((size_t)cells);
    std::vector<float> ang((size_t)cells), score((size_t)cells);
    std::vector<uint8_t> desc(32 * (size_t)cells);
    for (int i = 0; i < m; ++i) {
        const Feature *ft = f->_features[i];
        px[2 * (size_t)i] = ft->_pixel[0]; px[2 * (size_t)i + 1] = ft->_pixel[1]; lvl[(size_t)i] = ft->_level; ang[(size_t)i] = (float)ft->_angle;
    }
    if (ygz_hip_describe_given_angle(rt.ctx(), slot, px.data(), lvl.data(), ang.data(), m) != YGZ_OK) return false;
    ygz_kpt_soa out = { px.data(), lvl.data(), score.data(), ang.data(), desc.data() };
    int n = 0;
    if (ygz_hip_get_keypoints(rt.ctx(), slot, &out, cells, &n) != YGZ_OK || n != m) return false;
    for (int i = 0; i < m; ++i) {
        Feature *ft = f->_features[i];
        if (px[2 * (size_t)i] != ft->_pixel[0] || px[2 * (size_t)i + 1] != ft->_pixel[1] || lvl[(size_t)i] != ft->_level) return false;
        memcpy(ft->_desc.data, &desc[32 * (size_t)i], 32);
    }
    return true;
}

static bool build(World &w, Files &in)
{
    Memory::Clean();
    for (int k = 0; k < NK; ++k) {
        Frame *f = new Frame;
        Memory::RegisterKeyFrame(f);
        f->_id = f->_keyframe_id;
        f->_is_keyframe = true;
        f->_TCW = SE3::from7(&in.kf_poses[7 * (size_t)k]);
        w.kfs.push_back(f);
    }
    for (size_t p = 0; p < in.mp_pos.size() / 3; ++p) {
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_pos_world = Vector3d(in.mp_pos[3 * p], in.mp_pos[3 * p + 1], in.mp_pos[3 * p + 2]);
        mp->_cnt_visible = mp->_cnt_found = 1;
        w.index[mp] = (int32_t)w.mps.size();
        w.mps.push_back(mp);
    }
    for (size_t i = 0; i < in.kft_kf.size(); ++i) {
        Frame *fr = w.kfs[(size_t)in.kft_kf[i]];
        Feature *f = new Feature(Vector2d(in.kft_px[2 * i], in.kft_px[2 * i + 1]), in.kft_level[i]);
        f->_frame = fr;
        memcpy(f->_desc.data, &in.kft_desc[32 * i], 32);
        if (in.kft_mp[i] >= 0) {
            MapPoint *mp = w.mps[(size_t)in.kft_mp[i]];
            f->_mappoint = mp;
            if (mp->_obs.empty()) mp->_first_seen = mp->_last_seen = fr->_keyframe_id;
            mp->_obs[fr->_keyframe_id] = f;
        }
        fr->_features.push_back(f);
    }
    for (int k = 0; k < NF; ++k) {
        FrameIn &q = in.fr[k];
        Frame *f = new Frame;
        f->_id = 1000 + (unsigned long)k;
        f->_color = cv::Mat(H, W, CV_8UC1, q.img.data());
        f->InitFrame();
        f->_TCW = SE3::from7(q.pose.data());
        for (size_t i = 0; i < q.level.size(); ++i) {
            Feature *ft = new Feature(Vector2d(q.px[2 * i], q.px[2 * i + 1]), q.level[i]);
            ft->_frame = f; ft->_angle = q.angle[i]; ft->_depth = q.depth[i];
            if (q.mp[i] >= 0) ft->_mappoint = w.mps[(size_t)q.mp[i]];
            f->_features.push_back(ft);
        }
        w.frames.push_back(f);
        if (f->_pyramid.size() != 3 || !describe(f)) return false;
    }
    w.list_a = { w.kfs[0], w.kfs[1], w.kfs[2] };
    w.list_b = { w.kfs[1], w.kfs[2] };
    return true;
}

static bool dump(const std::string &s, const World &w, const std::vector<int32_t> &ret)
{
    std::vector<double> pose(7 * NF);
    std::vector<int32_t> mp;
    for (int k = 0; k < NF; ++k) {
        const Frame *f = w.frames[(size_t)k];
        f->_TCW.to7(&pose[7 * (size_t)k]);
        std::vector<int32_t> feat;
        std::vector<uint8_t> bad;
        std::vector<double> depth;
        for (const Feature *ft : f->_features) {
            const auto it = w.index.find(ft->_mappoint);
            feat.push_back(ft->_mappoint ? (it == w.index.end() ? -2 : it->second) : -1);
            bad.push_back(ft->_bad ? 1 : 0);
            depth.push_back(ft->_depth);
        }
        const std::string t = std::to_string(k);
        if (!put(s + "_feat" + t, feat) || !put(s + "_bad" + t, bad) || !put(s + "_depth" + t, depth)) return false;
    }
    for (const MapPoint *m : w.mps) { mp.push_back(m->_cnt_visible); mp.push_back(m->_cnt_found); mp.push_back(m->_track_in_view ? 1 : 0); }
    return put(s + "_pose", pose) && put(s + "_mp", mp) && put(s + "_ret", ret);
}

static std::vector<int32_t> flat(int ret, const std::vector<StereoLocalMap::Result> &res)
{
    std::vector<int32_t> o(1, ret);
    for (const StereoLocalMap::Result &r : res) o.insert(o.end(), { r.status, r.new_matches, r.edges, r.inliers, r.tracked ? 1 : 0 });
    return o;
}

static int run()
{
    Config::Set("image.width", "320"); Config::Set("image.height", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Files in;
    if (!read_all(in)) return 10;
    bool untouched = true;
    const size_t P = in.mp_pos.size() / 3;
    {   // old: the host-array route, frame by frame
        World w;
        if (!build(w, in)) return 11;
        const unsigned long next_id = Memory::CreateMapPoint()->_id + 1;
        StereoTracker tr;
        PoseOptimizer opt;
        std::vector<int32_t> ret;
        for (int k = 0; k < NF; ++k) {
            std::vector<double> ur;
            PoseOptimizer::URightFromDepth(w.frames[(size_t)k], tr._options._baseline, &ur);
            tr.SetURight(w.frames[(size_t)k], ur);
            ret.push_back(tr.TrackLocalMap(w.frames[(size_t)k], k < 3 ? w.list_a : w.list_b, opt));
        }
        if (!dump("old", w, ret)) return 12;
        untouched = untouched && Memory::GetNumberFrames() == NK && Memory::CreateMapPoint()->_id == next_id && w.mps.size() == P;
    }
    {   // batch: one call
        World w;
        if (!build(w, in)) return 13;
        const unsigned long next_id = Memory::CreateMapPoint()->_id + 1;
        StereoLocalMap lm;
        std::vector<StereoLocalMap::Result> res;
        // nothing to track: nothing is written
        if (lm.TrackLocalMap({}, {}, &res) != 0 || lm.TrackLocalMap({ w.frames[0] }, {}, &res) != 0 ||
            lm.TrackLocalMap({ w.frames[0], w.frames[0] }, { &w.list_a, &w.list_a }, &res) != 0 ||
            lm.TrackLocalMap({ w.frames[0], nullptr }, { &w.list_a, &w.list_a }, &res) != 0 || !res.empty())
            return 14;
        const int ret = lm.TrackLocalMap(w.frames, { &w.list_a, &w.list_a, &w.list_a, &w.list_b }, &res);
        if (res.size() != (size_t)NF || !dump("batch", w, flat(ret, res))) return 15;
        untouched = untouched && Memory::GetNumberFrames() == NK && Memory::CreateMapPoint()->_id == next_id && w.mps.size() == P;
    }
    {   // single: frame 1 alone
        World w;
        if (!build(w, in)) return 16;
        StereoLocalMap lm;
        std::vector<StereoLocalMap::Result> res;
        const int ret = lm.TrackLocalMap({ w.frames[1] }, { &w.list_a }, &res);
        if (res.size() != 1 || !dump("single", w, flat(ret, res))) return 17;
    }
    Memory::Clean();
    if (!put("untouched", std::vector<int32_t>(1, untouched ? 1 : 0))) return 18;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: slm_surface <dir>\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = run();
    } catch (const std::exception &ex) {
        fprintf(stderr, "slm_surface: %s\n", ex.what());
        return 4;
    }
    printf("slm_surface: %d\n", rc);
    return rc;
}
