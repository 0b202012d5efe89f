// ygz::StereoOdometry with more distinct frames in one call than the runtime keeps resident, a stand-alone program for
// tests/test_gpu_svo_residency.py (which runs it with YGZ_HIP_MAX_FRAMES=2): written against include/ygz only.
//   svo_resident <dir>
// reads what svo_surface reads: three QVGA gray pictures img0 .. img2 (uint8 [240][320]), per frame k its features k<k>_px (float64 [n][2]),
// k<k>_level (int32 [n]), k<k>_angle, k<k>_depth (float64 [n]) and pose0 (float64 [7]), the first frame's world -> camera pose.  Scenarios:
//   refused  TrackPairs over (1, 0), (2, 1): three distinct frames, the shared slot loader refuses them
//   single   Track(1, 0) afterwards: two frames, the normal path
// Written to <dir>: refused (int32 [2]: the return value, the length of the results), before_poses, refused_poses, single_poses (float64 [3][7]:
// every frame's _TCW at the start, after the refusal, at the end), single_res (int32 [6]: the return value, status, matches, inliers, retried,
// pose_written), single_match (int32 per feature of frame 0).
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include <cstdio>
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

static bool put_poses(const std::string &name, Frame *f)
{
    std::vector<double> poses(21);
    for (int k = 0; k < 3; ++k) f[k]._TCW.to7(&poses[7 * k]);
    return put(name, poses);
}

static int run()
{
    Config::Set("image.width", "320"); Config::Set("image.height", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Input in[3];
    std::vector<double> pose0;
    for (int k = 0; k < 3; ++k) {
        const std::string s = std::to_string(k);
        Input &q = in[k];
        if (!get("img" + s, q.img) || q.img.size() != (size_t)W * H || !get("k" + s + "_px", q.px) || !get("k" + s + "_level", q.level) ||
            !get("k" + s + "_angle", q.angle) || !get("k" + s + "_depth", q.depth) || q.px.size() != 2 * q.level.size() ||
            q.angle.size() != q.level.size() || q.depth.size() != q.level.size() || q.level.empty())
            return 10;
    }
    if (!get("pose0", pose0) || pose0.size() != 7) return 11;
    Frame f[3];
    for (int k = 0; k < 3; ++k) {
        f[k]._color = cv::Mat(H, W, CV_8UC1, in[k].img.data());
        f[k].InitFrame();
        if (f[k]._pyramid.size() != 3) return 12;
        for (size_t i = 0; i < in[k].level.size(); ++i) {
            Feature *ft = new Feature(Vector2d(in[k].px[2 * i], in[k].px[2 * i + 1]), in[k].level[i]);
            ft->_frame = &f[k]; ft->_angle = in[k].angle[i]; ft->_depth = in[k].depth[i];
            f[k]._features.push_back(ft);
        }
    }
    f[0]._TCW = SE3::from7(pose0.data());
    if (!put_poses("before_poses", f)) return 13;

    StereoOdometry::Options o;
    o._min_matches = 6; o._min_tracked = 3;                              // a dozen features per frame
    StereoOdometry od(o);
    std::vector<StereoOdometry::Result> res(5);
    const int refused = od.TrackPairs({ { &f[1], &f[0] }, { &f[2], &f[1] } }, nullptr, &res);
    if (!put("refused", std::vector<int32_t>{ refused, (int32_t)res.size() }) || !put_poses("refused_poses", f)) return 14;

    StereoOdometry::Result one;
    const bool ok = od.Track(&f[1], &f[0], SE3(), &one);
    const std::vector<int32_t> r = { ok ? 1 : 0, one.status, one.matches, one.inliers, one.retried, one.pose_written ? 1 : 0 };
    if (!put("single_res", r) || !put("single_match", one.match) || !put_poses("single_poses", f)) return 15;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: svo_resident <dir>\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = run();
    } catch (const std::exception &ex) {
        fprintf(stderr, "svo_resident: %s\n", ex.what());
        return 4;
    }
    printf("svo_resident: %d\n", rc);
    return rc;
}
