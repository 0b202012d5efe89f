// ygz::StereoMatcher (include/ygz/Algorithm/StereoMatcher.h), a stand-alone program for tests/test_gpu_stereo_surface.py: written against
// include/ygz only.
//   stereo_surface <dir>     reads <dir>/left.bin, right.bin (320 x 240 gray) and the two keypoint lists <dir>/{l,r}_{px,level,desc}.bin (float64
//        [n][2], int32 [n], uint8 [n][32]) that the test wrote; two frames are initialised and given those features; ComputeStereoMatches runs
//        with a baseline of 0.25 m; then the array form ygz_hip_stereo_match runs on the same arrays and slots.
// Written to <dir>: depth.bin (Feature::_depth of every left feature afterwards; -1 is what it was before), u_right.bin, status.bin, count.bin
// (the return value and the number of left features), abi_depth.bin, abi_u_right.bin, abi_status.bin, fx.bin (the camera's float fx).
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <cstdio>
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

struct List { std::vector<double> px; std::vector<int32_t> level; std::vector<uint8_t> desc; };

static bool read_list(const std::string &side, List &k)
{
    return get(side + "_px", k.px) && get(side + "_level", k.level) && get(side + "_desc", k.desc) && k.px.size() == 2 * k.level.size() &&
           k.desc.size() == 32 * k.level.size();
}

static void give(Frame &f, const List &k)
{
    for (size_t i = 0; i < k.level.size(); ++i) {
        Feature *ft = new Feature(Vector2d(k.px[2 * i], k.px[2 * i + 1]), k.level[i]);
        memcpy(ft->_desc.data, &k.desc[32 * i], 32);
        ft->_frame = &f;
        f._features.push_back(ft);
    }
}

static int run()
{
    const int W = 320, H = 240;
    Config::Set("image.width", "320"); Config::Set("image.height", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    std::vector<uint8_t> left, right;
    List kl, kr;
    if (!get("left", left) || !get("right", right) || left.size() != (size_t)W * H || right.size() != left.size()) return 10;
    if (!read_list("l", kl) || !read_list("r", kr) || kl.level.empty() || kr.level.empty()) return 11;
    Frame fl, fr;
    fl._color = cv::Mat(H, W, CV_8UC1, left.data());
    fl.InitFrame();
    fr._color = cv::Mat(H, W, CV_8UC1, right.data());
    fr.InitFrame();
    if (fl._pyramid.size() != 3 || fr._pyramid.size() != 3) return 12;
    give(fl, kl);
    give(fr, kr);

    StereoMatcher::Options opt;
    opt._baseline = 0.25;
    StereoMatcher sm(opt);
    // nothing to match against: nothing is set
    if (sm.ComputeStereoMatches(&fl, nullptr) != 0 || sm.ComputeStereoMatches(&fl, &fl) != 0 || sm.ComputeStereoMatches(nullptr, &fr) != 0) return 13;
    for (const Feature *ft : fl._features) if (ft->_depth != -1) return 14;

    std::vector<double> u_right;
    const int n = (int)kl.level.size();
    const int set = sm.ComputeStereoMatches(&fl, &fr, &u_right);
    if ((int)u_right.size() != n || (int)sm.GetStatus().size() != n) return 15;
    std::vector<double> depth((size_t)n);
    for (int i = 0; i < n; ++i) depth[i] = fl._features[i]->_depth;
    for (const Feature *ft : fr._features) if (ft->_depth != -1) return 16;          // the right frame's features are read only
    std::vector<int32_t> status(sm.GetStatus().begin(), sm.GetStatus().end()), count = { set, n };
    if (!put("depth", depth) || !put("u_right", u_right) || !put("status", status) || !put("count", count)) return 17;

    // the array form on the same arrays and slots
    hip::Runtime &rt = hip::Runtime::Get();
    const int sl = rt.Resident(&fl), sr = rt.Resident(&fr);
    if (sl < 0 || sr < 0 || sl == sr) return 18;
    ygz_stereo_params p;
    ygz_hip_default_stereo_params(&p);
    p.baseline = 0.25;
    std::vector<double> a_depth((size_t)n), a_ur((size_t)n);
    std::vector<int32_t> a_status((size_t)n);
    if (ygz_hip_stereo_match(rt.ctx(), sl, sr, kl.px.data(), kl.level.data(), kl.desc.data(), n, kr.px.data(), kr.level.data(), kr.desc.data(),
                             (int)kr.level.size(), &p, nullptr, a_ur.data(), a_depth.data(), nullptr, a_status.data(), nullptr) != YGZ_OK) return 19;
    const std::vector<float> fx = { cam.fx() };
    if (!put("abi_depth", a_depth) || !put("abi_u_right", a_ur) || !put("abi_status", a_status) || !put("fx", fx)) return 20;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: stereo_surface <dir>\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = run();
    } catch (const std::exception &ex) {
        fprintf(stderr, "stereo_surface: %s\n", ex.what());
        return 4;
    }
    printf("stereo_surface: %d\n", rc);
    return rc;
}
