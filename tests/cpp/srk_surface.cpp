// ygz::StereoRefTracker (include/ygz/Algorithm/StereoRefTracker.h), a stand-alone program for tests/test_srk_surface_build.py and
// tests/test_gpu_srk_surface.py: written against include/ygz only.
//   srk_surface <dir>
// reads a small stereo map: a vocabulary (vocab, DBoW3's binary format), two keyframes and four frames, each with a QVGA gray picture
// k<j>_img / f<k>_img (uint8 [240][320]), its features _px (float64 [n][2]), _level (int32 [n]), _angle, _depth (float64 [n]; <= 0: none) and
// its pose _pose (float64 [7]; a frame's is its entry pose); a keyframe's features also have k<j>_mp (int32 [n]: the map point or -1); the map
// points mp_pos (float64 [P][3]).  Frames 0 and 1 are tracked against keyframe 0, frames 2 and 3 against keyframe 1.  A feature's _desc is
// what the device describes at its pixel, so that the host-array route sees the descriptors the resident route computes.  Scenarios, each on
// a fresh copy of the map:
//   old     per frame in order: every _mappoint cleared, Matcher::SearchByBoW(keyframe, frame) with checkOrientation off, th_low 50 and
//           knnRatio 0.7, the claim of ygz_reloc.cpp (a frame feature goes to the first keyframe feature with a good point that names it);
//           with at least 15 associations: _mappoint, PoseOptimizer::Optimize with PoseOptimizer::URightFromDepth (the points' _cnt_found
//           saved and restored), a _bad feature loses its _mappoint
//   batch   ONE StereoRefTracker::TrackReferenceKeyFrame over the four frames, _check_orientation off
//   single  StereoRefTracker::TrackReferenceKeyFrame of frame 1 alone
// Written to <dir>: per scenario <s>: <s>_pose (float64 [4][7]), <s>_feat<k> (int32 per feature: the map point's index or -1), <s>_bad<k> (uint8),
// <s>_depth<k> (float64), <s>_found (int32 [P]: _cnt_found), <s>_ret (int32: old: per frame the associations and the features kept; batch,
// single: the return value, then per frame status, matches, inliers, kept, tracked); untouched (int32: 1 when no scenario made a map point or
// a keyframe); nodes (int32: the distinct FeatureVector nodes of keyframe 0 at levelsup 4).
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
static const int W = 320, H = 240, NF = 4, NK = 2;
static const int KF_OF[NF] = { 0, 0, 1, 1 };

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
struct Files { FrameIn kf[NK], fr[NF]; std::vector<double> mp_pos; std::vector<uint8_t> vocab; };

static bool read_frame(const std::string &s, FrameIn &f, bool keyframe)
{
    return get(s + "_img", f.img) && f.img.size() == (size_t)W * H && get(s + "_px", f.px) && get(s + "_level", f.level) &&
           get(s + "_angle", f.angle) && get(s + "_depth", f.depth) && get(s + "_pose", f.pose) && (!keyframe || get(s + "_mp", f.mp)) &&
           f.px.size() == 2 * f.level.size() && f.angle.size() == f.level.size() && f.depth.size() == f.level.size() &&
           (!keyframe || f.mp.size() == f.level.size()) && f.pose.size() == 7 && !f.level.empty();
}

static bool read_all(Files &in)
{
    for (int k = 0; k < NK; ++k) if (!read_frame("k" + std::to_string(k), in.kf[k], true)) return false;
    for (int k = 0; k < NF; ++k) if (!read_frame("f" + std::to_string(k), in.fr[k], false)) return false;
    return get("mp_pos", in.mp_pos) && get("vocab", in.vocab) && !in.vocab.empty();
}

struct World {
    std::vector<Frame *> kfs, frames;
    std::vector<MapPoint *> mps;
    std::map<const MapPoint *, int32_t> index;
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

static Frame *make_frame(FrameIn &q, unsigned long id)
{
    Frame *f = new Frame;
    f->_id = id;
    f->_color = cv::Mat(H, W, CV_8UC1, q.img.data());
    f->InitFrame();
    f->_TCW = SE3::from7(q.pose.data());
    for (size_t i = 0; i < q.level.size(); ++i) {
        Feature *ft = new Feature(Vector2d(q.px[2 * i], q.px[2 * i + 1]), q.level[i]);
        ft->_frame = f; ft->_angle = q.angle[i]; ft->_depth = q.depth[i];
        f->_features.push_back(ft);
    }
    return f;
}

static bool build(World &w, Files &in)
{
    Memory::Clean();
    for (size_t p = 0; p < in.mp_pos.size() / 3; ++p) {
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_pos_world = Vector3d(in.mp_pos[3 * p], in.mp_pos[3 * p + 1], in.mp_pos[3 * p + 2]);
        mp->_cnt_visible = mp->_cnt_found = 1;
        w.index[mp] = (int32_t)w.mps.size();
        w.mps.push_back(mp);
    }
    for (int k = 0; k < NK; ++k) {
        Frame *f = make_frame(in.kf[k], 500 + (unsigned long)k);
        Memory::RegisterKeyFrame(f);
        f->_is_keyframe = true;
        w.kfs.push_back(f);
        for (size_t i = 0; i < f->_features.size(); ++i) {
            const int32_t p = in.kf[k].mp[i];
            if (p < 0) continue;
            MapPoint *mp = w.mps[(size_t)p];
            f->_features[i]->_mappoint = mp;
            if (mp->_obs.empty()) mp->_first_seen = mp->_last_seen = f->_keyframe_id;
            mp->_obs[f->_keyframe_id] = f->_features[i];
        }
        if (f->_pyramid.size() != 3 || !describe(f)) return false;
    }
    for (int k = 0; k < NF; ++k) {
        Frame *f = make_frame(in.fr[k], 1000 + (unsigned long)k);
        w.frames.push_back(f);
        if (f->_pyramid.size() != 3 || !describe(f)) return false;
    }
    return true;
}

static bool dump(const std::string &s, const World &w, const std::vector<int32_t> &ret)
{
    std::vector<double> pose(7 * NF);
    std::vector<int32_t> found;
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
    for (const MapPoint *m : w.mps) found.push_back(m->_cnt_found);
    return put(s + "_pose", pose) && put(s + "_found", found) && put(s + "_ret", ret);
}

static std::vector<int32_t> flat(int ret, const std::vector<StereoRefTracker::Result> &res)
{
    std::vector<int32_t> o(1, ret);
    for (const StereoRefTracker::Result &r : res) o.insert(o.end(), { r.status, r.matches, r.inliers, r.kept, r.tracked ? 1 : 0 });
    return o;
}

// the host route for one frame: (associations, features kept)
static std::pair<int, int> old_route(Frame *kf, Frame *cur, Matcher &matcher, PoseOptimizer &opt)
{
    for (Feature *ft : cur->_features) ft->_mappoint = nullptr;
    kf->ComputeBoW();
    cur->ComputeBoW();
    std::map<int, int> matches;
    matcher.SearchByBoW(kf, cur, matches);
    std::vector<char> used(cur->_features.size(), 0);
    std::vector<std::pair<int, MapPoint *>> got;
    for (const auto &m : matches) {
        if (m.first < 0 || m.first >= (int)kf->_features.size() || m.second < 0 || m.second >= (int)cur->_features.size() || used[m.second]) continue;
        MapPoint *mp = kf->_features[m.first]->_mappoint;
        if (!mp || mp->_bad) continue;
        used[m.second] = 1;
        got.push_back(std::make_pair(m.second, mp));
    }
    if ((int)got.size() < 15) return std::make_pair((int)got.size(), 0);
    std::vector<int> found;
    for (const auto &g : got) { cur->_features[(size_t)g.first]->_mappoint = g.second; found.push_back(g.second->_cnt_found); }
    std::vector<double> ur;
    PoseOptimizer::URightFromDepth(cur, opt._options._baseline, &ur);
    opt.Optimize(cur, &ur);
    for (size_t k = got.size(); k-- > 0;) got[k].second->_cnt_found = found[k];
    int kept = 0;
    for (Feature *ft : cur->_features) {
        if (ft->_bad) ft->_mappoint = nullptr;
        if (ft->_mappoint && !ft->_mappoint->_bad && !ft->_mappoint->_obs.empty()) ++kept;
    }
    return std::make_pair((int)got.size(), kept);
}

static int run()
{
    Config::Set("image.width", "320"); Config::Set("image.height", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Files in;
    if (!read_all(in)) return 10;
    ORBVocabulary voc;
    if (!voc.loadFromMemory(in.vocab.data(), in.vocab.size())) return 9;
    Frame::SetORBVocabulary(&voc);
    bool untouched = true;
    const size_t P = in.mp_pos.size() / 3;
    StereoRefTracker::Options o;
    o._check_orientation = false;
    {   // old: the host-array route, frame by frame
        World w;
        if (!build(w, in)) return 11;
        const unsigned long next_id = Memory::CreateMapPoint()->_id + 1;
        Matcher matcher;
        matcher._options.th_low = 50; matcher._options.knnRatio = 0.7f; matcher._options.checkOrientation = false;
        PoseOptimizer opt;
        std::vector<int32_t> ret;
        for (int k = 0; k < NF; ++k) {
            const std::pair<int, int> r = old_route(w.kfs[(size_t)KF_OF[k]], w.frames[(size_t)k], matcher, opt);
            ret.push_back(r.first); ret.push_back(r.second);
        }
        if (!dump("old", w, ret)) return 12;
        if (!put("nodes", std::vector<int32_t>(1, (int32_t)w.kfs[0]->_feature_vec.size()))) return 12;
        untouched = untouched && Memory::GetNumberFrames() == NK && Memory::CreateMapPoint()->_id == next_id && w.mps.size() == P;
    }
    {   // batch: one call
        World w;
        if (!build(w, in)) return 13;
        const unsigned long next_id = Memory::CreateMapPoint()->_id + 1;
        StereoRefTracker tr(o);
        std::vector<StereoRefTracker::Result> res;
        // nothing to track: nothing is written
        if (tr.TrackReferenceKeyFrame({}, {}, &res) != 0 || tr.TrackReferenceKeyFrame({ w.frames[0] }, {}, &res) != 0 ||
            tr.TrackReferenceKeyFrame({ w.frames[0], w.frames[0] }, { w.kfs[0], w.kfs[0] }, &res) != 0 ||
            tr.TrackReferenceKeyFrame({ w.frames[0], nullptr }, { w.kfs[0], w.kfs[0] }, &res) != 0 ||
            tr.TrackReferenceKeyFrame({ w.frames[0] }, { nullptr }, &res) != 0 || tr.TrackReferenceKeyFrame({ w.kfs[0] }, { w.kfs[0] }, &res) != 0 ||
            !res.empty())
            return 14;
        const int ret = tr.TrackReferenceKeyFrame(w.frames, { w.kfs[0], w.kfs[0], w.kfs[1], w.kfs[1] }, &res);
        if (res.size() != (size_t)NF || !dump("batch", w, flat(ret, res))) return 15;
        untouched = untouched && Memory::GetNumberFrames() == NK && Memory::CreateMapPoint()->_id == next_id && w.mps.size() == P;
    }
    {   // single: frame 1 alone
        World w;
        if (!build(w, in)) return 16;
        StereoRefTracker tr(o);
        std::vector<StereoRefTracker::Result> res;
        const int ret = tr.TrackReferenceKeyFrame({ w.frames[1] }, { w.kfs[0] }, &res);
        if (res.size() != 1 || !dump("single", w, flat(ret, res))) return 17;
    }
    Memory::Clean();
    Frame::SetORBVocabulary(nullptr);
    if (!put("untouched", std::vector<int32_t>(1, untouched ? 1 : 0))) return 18;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: srk_surface <dir>\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = run();
    } catch (const std::exception &ex) {
        fprintf(stderr, "srk_surface: %s\n", ex.what());
        return 4;
    }
    printf("srk_surface: %d\n", rc);
    return rc;
}
