// Frame::InitFrame through the lens undistortion (include/ygz/Basic/{Camera,Frame}.h, ygz::hip::Runtime::UploadColor), a stand-alone program for
// tests/test_gpu_undistort_surface.py: written against include/ygz only.
//   undist_surface <out_dir> distorted   camera.k1, k2, p1, p2 set (TUM fr1), 160 x 120, two slots (YGZ_HIP_MAX_FRAMES=2 in the environment):
//        a BGR frame and a gray frame initialised, level 0 and 1 taken; the gray frame's _pyramid[0] fetched and its _color released; two more
//        frames evict both; both come back (the first from _color: undistorted again, the second from the _pyramid[0] mirror: uploaded as it
//        is) and their levels are taken again
//   undist_surface <out_dir> default     the default configuration: no coefficient, _pyramid[0] of a BGR frame
// Every image goes to <out_dir>/<name>.bin as raw bytes; the test compares them with the restatement.
#include "ygz/Basic.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace ygz;

static std::string g_dir;

static bool put(const std::string &name, const uint8_t *p, size_t n)
{
    FILE *f = fopen((g_dir + "/" + name + ".bin").c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// a picture with structure at every scale from a 32-bit LCG: waves plus noise
static std::vector<uint8_t> picture(int w, int h, int ch, uint32_t seed)
{
    std::vector<uint8_t> v((size_t)w * h * ch);
    uint32_t s = seed;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            for (int c = 0; c < ch; ++c) {
                s = s * 1664525u + 1013904223u;
                const int wave = ((x * 5 + y * 3 + c * 40) & 127) + ((x / 9 + y / 7) & 1) * 60;
                v[((size_t)y * w + x) * ch + c] = (uint8_t)((wave + (int)((s >> 24) & 63)) & 255);
            }
    return v;
}

static bool device_level(Frame *f, int level, std::vector<uint8_t> &out)
{
    hip::Runtime &rt = hip::Runtime::Get();
    const int slot = rt.Resident(f);
    int w = 0, h = 0;
    if (slot < 0 || ygz_hip_level_size(rt.ctx(), level, &w, &h) != YGZ_OK) return false;
    out.assign((size_t)w * h, 0);
    return ygz_hip_download_level(rt.ctx(), slot, level, out.data()) == YGZ_OK;
}

static bool take(Frame *f, const std::string &name)
{
    std::vector<uint8_t> l0, l1;
    return device_level(f, 0, l0) && device_level(f, 1, l1) && put(name + "_l0", l0.data(), l0.size()) && put(name + "_l1", l1.data(), l1.size());
}

static int run_default()
{
    const int W = 640, H = 480;
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    if (cam.HasDistortion()) return 10;
    std::vector<uint8_t> a = picture(W, H, 3, 7u);
    Frame f;
    f._color = cv::Mat(H, W, CV_8UC3, a.data());
    f.InitFrame();
    if (f._pyramid.size() != 3 || f._pyramid[0].empty()) return 11;
    if (!put("default_color", a.data(), a.size()) || !put("default_l0", f._pyramid[0].data, (size_t)W * H)) return 12;
    // no map was set: the undistorting call is refused
    if (ygz_hip_build_pyramid_undistorted(hip::Runtime::Get().ctx(), 0, 1, 1) != YGZ_E_STATE) return 13;
    return 0;
}

static int run_distorted()
{
    const int W = 160, H = 120;
    Config::Set("image.width", "160"); Config::Set("image.height", "120");
    Config::Set("camera.fx", "130.2"); Config::Set("camera.fy", "130.3"); Config::Set("camera.cx", "81.3"); Config::Set("camera.cy", "62.4");
    Config::Set("camera.k1", "0.2624"); Config::Set("camera.k2", "-0.9531"); Config::Set("camera.p1", "-0.0054"); Config::Set("camera.p2", "0.0026");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    if (!cam.HasDistortion() || cam.k1() != 0.2624f || cam.k2() != -0.9531f || cam.p1() != -0.0054f || cam.p2() != 0.0026f) return 20;
    const float coeff[8] = { cam.k1(), cam.k2(), cam.p1(), cam.p2(), cam.fx(), cam.fy(), cam.cx(), cam.cy() };
    if (!put("camera", (const uint8_t *)coeff, sizeof(coeff))) return 21;
    const Vector2d d = cam.DistortPoint(Vector2d(0.31, -0.22));
    const double dd[2] = { d[0], d[1] };
    if (!put("distort_point", (const uint8_t *)dd, sizeof(dd))) return 21;

    std::vector<uint8_t> a = picture(W, H, 3, 1u), b = picture(W, H, 1, 2u), c = picture(W, H, 3, 3u), e = picture(W, H, 1, 4u);
    if (!put("a_color", a.data(), a.size()) || !put("b_color", b.data(), b.size())) return 22;
    Frame fa, fb, fc, fe;
    fa._color = cv::Mat(H, W, CV_8UC3, a.data());
    fa.InitFrame();
    if (fa._pyramid.size() != 3 || !take(&fa, "a_before")) return 23;
    if (!put("a_mirror_l0", fa._pyramid[0].data, (size_t)W * H)) return 23;
    fb._color = cv::Mat(H, W, CV_8UC1, b.data());
    fb.InitFrame();
    if (fb._pyramid.size() != 3 || !take(&fb, "b_before")) return 24;
    if (fb._pyramid[0].empty()) return 24;             // the mirror of level 0 is fetched ...
    fb._color = cv::Mat();                             // ... and the picture released: the frame can only come back from the mirror
    // two more frames take both slots
    fc._color = cv::Mat(H, W, CV_8UC3, c.data());
    fc.InitFrame();
    fe._color = cv::Mat(H, W, CV_8UC1, e.data());
    fe.InitFrame();
    if (fa._hip_slot >= 0 || fb._hip_slot >= 0 || fc._hip_slot < 0 || fe._hip_slot < 0) return 25;      // both evicted
    if (!take(&fa, "a_after")) return 26;              // from _color: uploaded and undistorted again
    if (!take(&fb, "b_after")) return 27;              // from the _pyramid[0] mirror: already undistorted, uploaded as it is
    if (fa._hip_slot < 0 || fb._hip_slot < 0) return 28;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: undist_surface <out_dir> distorted|default\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = strcmp(argv[2], "default") == 0 ? run_default() : run_distorted();
    } catch (const std::exception &ex) {
        fprintf(stderr, "undist_surface: %s\n", ex.what());
        return 4;
    }
    printf("undist_surface %s: %d\n", argv[2], rc);
    return rc;
}
