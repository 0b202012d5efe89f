// ygz::StereoOdometry (include/ygz/Algorithm/StereoOdometry.h), a stand-alone program for tests/test_svo_surface_build.py and
// tests/test_gpu_svo_surface.py: written against include/ygz only.
//   svo_surface <dir>
// reads three QVGA gray pictures of a sequence, img0 .. img2 (uint8 [240][320]), per frame k its features k<k>_px (float64 [n][2]), k<k>_level
// (int32 [n]), k<k>_angle, k<k>_depth (float64 [n]; <= 0: none) and pose0 (float64 [7]), the first frame's world -> camera pose.  Five frames
// are built: 0, 1, 2 of the sequence, a copy of frame 2, and a copy of frame 0 without any depth.  Scenarios:
//   batch   TrackPairs over (1, 0), (2, 1) and (copy of 2, blind copy of 0) without guesses: the third pair cannot be tracked
//   abi     ygz_hip_stereo_odometry_slots on the slots the batch left, same parameters
//   strict  TrackPairs over (1, 0), (2, 1) with _min_tracked above every inlier count, on fresh poses: no pose is written
//   single  Track(1, 0) on fresh poses
// Written to <dir>: per scenario <s> in batch, strict, single: <s>_res (int32 [pairs][5]: status, matches, inliers, retried, pose_written),
// <s>_trel (float64 [pairs][7]), <s>_match<p> (int32 per feature of pair p's last frame), <s>_poses (float64 [5][7]: every frame's _TCW
// afterwards), <s>_ret (int32: the return value); abi_trel, abi_status, abi_counts [3][8], abi_inliers, abi_match [3][cells]; untouched (int32:
// 1 when no feature of any frame has a _mappoint, every feature list kept its length, Memory holds no keyframe and no map point was made).
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
static const int W = 320, H = 240;

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

struct Input { std::vector<uint8_t> img; std::vector<double> px, angle, depth; std::vector<int32_t> level; };

static bool read_frame(int k, Input &in)
{
    const std::string s = std::to_string(k);
    return get("img" + s, in.img) && in.img.size() == (size_t)W * H && get("k" + s + "_px", in.px) && get("k" + s + "_level", in.level) &&
           get("k" + s + "_angle", in.angle) && get("k" + s + "_depth", in.depth) && in.px.size() == 2 * in.level.size() &&
           in.angle.size() == in.level.size() && in.depth.size() == in.level.size() && !in.level.empty();
}

static void build(Frame &f, Input &in, bool blind)
{
    f._color = cv::Mat(H, W, CV_8UC1, in.img.data());
    f.InitFrame();
    for (size_t i = 0; i < in.level.size(); ++i) {
        Feature *ft = new Feature(Vector2d(in.px[2 * i], in.px[2 * i + 1]), in.level[i]);
        ft->_frame = &f; ft->_angle = in.angle[i]; ft->_depth = blind ? -1.0 : in.depth[i];
        f._features.push_back(ft);
    }
}

struct World {
    Frame f[5];                                     // 0, 1, 2, a copy of 2, a blind copy of 0
    void reset(const std::vector<double> &pose0)
    {
        for (int k = 0; k < 5; ++k) f[k]._TCW = SE3();
        f[0]._TCW = SE3::from7(pose0.data());
        f[4]._TCW = SE3::from7(pose0.data());
    }
};

static bool dump(const std::string &s, World &w, const std::vector<StereoOdometry::Result> &res, int ret)
{
    std::vector<int32_t> r, rets(1, ret);
    std::vector<double> trel, poses(35);
    for (size_t p = 0; p < res.size(); ++p) {
        const StereoOdometry::Result &q = res[p];
        r.insert(r.end(), { q.status, q.matches, q.inliers, q.retried, q.pose_written ? 1 : 0 });
        double T[7];
        q.T_rel.to7(T);
        trel.insert(trel.end(), T, T + 7);
        if (!put(s + "_match" + std::to_string(p), q.match)) return false;
    }
    for (int k = 0; k < 5; ++k) w.f[k]._TCW.to7(&poses[7 * k]);
    return put(s + "_res", r) && put(s + "_trel", trel) && put(s + "_poses", poses) && put(s + "_ret", rets);
}

static int run()
{
    Config::Set("image.width", "320"); Config::Set("image.height", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Input in[3];
    std::vector<double> pose0;
    for (int k = 0; k < 3; ++k) if (!read_frame(k, in[k])) return 10;
    if (!get("pose0", pose0) || pose0.size() != 7) return 11;
    Memory::Clean();
    const unsigned long first_id = Memory::CreateMapPoint()->_id;          // the next point made gets the next id: none is made in between
    World w;
    const int src[5] = { 0, 1, 2, 2, 0 };
    for (int k = 0; k < 5; ++k) build(w.f[k], in[src[k]], k == 4);
    for (int k = 0; k < 5; ++k) if (w.f[k]._pyramid.size() != 3) return 12;

    StereoOdometry od;
    std::vector<StereoOdometry::Result> res;
    // nothing to track: nothing is written
    if (od.TrackPairs({}, nullptr, &res) != 0 || od.TrackPairs({ { &w.f[1], nullptr } }, nullptr, &res) != 0 ||
        od.TrackPairs({ { &w.f[1], &w.f[1] } }, nullptr, &res) != 0 || !res.empty())
        return 13;
    {   // batch
        w.reset(pose0);
        const int ret = od.TrackPairs({ { &w.f[1], &w.f[0] }, { &w.f[2], &w.f[1] }, { &w.f[3], &w.f[4] } }, nullptr, &res);
        if (res.size() != 3 || !dump("batch", w, res, ret)) return 14;
    }
    {   // abi: the same slots, the same parameters
        hip::Runtime &rt = hip::Runtime::Get();
        const int cells = rt.cells();
        int32_t last[3] = { rt.Resident(&w.f[0]), rt.Resident(&w.f[1]), rt.Resident(&w.f[4]) };
        int32_t cur[3] = { rt.Resident(&w.f[1]), rt.Resident(&w.f[2]), rt.Resident(&w.f[3]) };
        ygz_svo_params prm;
        ygz_hip_default_svo_params(&prm);
        std::vector<double> trel(21);
        std::vector<int32_t> status(3), counts(24), inliers(3), match(3 * (size_t)cells);
        if (ygz_hip_stereo_odometry_slots(rt.ctx(), 3, last, cur, nullptr, nullptr, &prm, trel.data(), status.data(), counts.data(), match.data(),
                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, inliers.data(),
                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != YGZ_OK)
            return 15;
        if (!put("abi_trel", trel) || !put("abi_status", status) || !put("abi_counts", counts) || !put("abi_inliers", inliers) ||
            !put("abi_match", match))
            return 16;
    }
    {   // strict
        w.reset(pose0);
        StereoOdometry::Options o;
        o._min_tracked = 1000000;
        StereoOdometry strict(o);
        const int ret = strict.TrackPairs({ { &w.f[1], &w.f[0] }, { &w.f[2], &w.f[1] } }, nullptr, &res);
        if (res.size() != 2 || !dump("strict", w, res, ret)) return 17;
    }
    {   // single
        w.reset(pose0);
        StereoOdometry::Result one;
        const bool ok = od.Track(&w.f[1], &w.f[0], SE3(), &one);
        if (!dump("single", w, std::vector<StereoOdometry::Result>(1, one), ok ? 1 : 0)) return 18;
    }
    bool untouched = Memory::GetNumberFrames() == 0 && Memory::CreateMapPoint()->_id == first_id + 1;
    for (int k = 0; k < 5; ++k) {
        untouched = untouched && w.f[k]._features.size() == in[src[k]].level.size();
        for (const Feature *ft : w.f[k]._features) untouched = untouched && ft->_mappoint == nullptr;
    }
    if (!put("untouched", std::vector<int32_t>(1, untouched ? 1 : 0))) return 19;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: svo_surface <dir>\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = run();
    } catch (const std::exception &ex) {
        fprintf(stderr, "svo_surface: %s\n", ex.what());
        return 4;
    }
    printf("svo_surface: %d\n", rc);
    return rc;
}
