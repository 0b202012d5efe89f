// ygz::StereoRig (include/ygz/Basic/StereoRig.h) in front of the stereo chain, a stand-alone program for tests/test_gpu_rectify_surface.py:
// written against include/ygz only.  The test writes <dir>/calib.bin (doubles: w, h, the output camera fx fy cx cy, the left and the right lens
// as fx fy cx cy k1 k2 p1 p2 k3, R [9], T [3], border value) and the pictures; the program writes rig.bin (R1 [9], R2 [9], Baseline, bf) and:
//   rect_surface <dir> bgr|gray   two slots (YGZ_HIP_MAX_FRAMES=2 in the environment): left.bin, right.bin go through InitPair, level 0 and 1 are
//        taken; the right frame's _pyramid[0] is fetched and its _color released; two plain frames (c.bin, e.bin: InitFrame) evict both and
//        their level 0 is taken; both rig frames come back (the left one from _color: rectified again, the right one from the _pyramid[0]
//        mirror: uploaded as it is) and their levels are taken again
//   rect_surface <dir> stereo     raw_left.bin, raw_right.bin (gray): InitPair, FeatureDetector::Detect on both, ComputeStereoMatches with
//        _baseline = rig.Baseline(); the features, the levels of both frames and depth.bin, u_right.bin, status.bin, count.bin are written
// Every image goes to <dir>/<name>.bin as raw bytes; the test compares them with the restatement.
#include "ygz/Basic.h"
#include "ygz/Basic/StereoRig.h"
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

template <typename T> static bool put(const std::string &name, const T *p, size_t n)
{
    FILE *f = fopen((g_dir + "/" + name + ".bin").c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, sizeof(T), n, f) == n;
    return fclose(f) == 0 && ok;
}

static std::string num(double v) { char b[64]; snprintf(b, sizeof(b), "%.9g", v); return b; }

static bool device_level(Frame *f, int level, std::vector<uint8_t> &out)
{
    hip::Runtime &rt = hip::Runtime::Get();
    const int slot = rt.Resident(f);
    int w = 0, h = 0;
    if (slot < 0 || ygz_hip_level_size(rt.ctx(), level, &w, &h) != YGZ_OK) return false;
    out.assign((size_t)w * h, 0);
    return ygz_hip_download_level(rt.ctx(), slot, level, out.data()) == YGZ_OK;
}

static bool take(Frame *f, const std::string &name, int levels = 2)
{
    for (int L = 0; L < levels; ++L) {
        std::vector<uint8_t> v;
        if (!device_level(f, L, v) || !put(name + "_l" + std::to_string(L), v.data(), v.size())) return false;
    }
    return true;
}

static int W = 0, H = 0;

// the configuration and the rig of calib.bin
static bool calibration(StereoRig::Calibration &cal)
{
    std::vector<double> c;
    if (!get("calib", c) || c.size() != 37) return false;
    W = (int)c[0]; H = (int)c[1];
    Config::Set("image.width", std::to_string(W)); Config::Set("image.height", std::to_string(H));
    Config::Set("camera.fx", num(c[2])); Config::Set("camera.fy", num(c[3])); Config::Set("camera.cx", num(c[4])); Config::Set("camera.cy", num(c[5]));
    StereoRig::Lens *lens[2] = { &cal.left, &cal.right };
    for (int k = 0; k < 2; ++k) {
        const double *l = &c[6 + 9 * k];
        lens[k]->fx = l[0]; lens[k]->fy = l[1]; lens[k]->cx = l[2]; lens[k]->cy = l[3];
        lens[k]->k1 = l[4]; lens[k]->k2 = l[5]; lens[k]->p1 = l[6]; lens[k]->p2 = l[7]; lens[k]->k3 = l[8];
    }
    for (int i = 0; i < 9; ++i) cal.R[i] = c[24 + i];
    for (int i = 0; i < 3; ++i) cal.T[i] = c[33 + i];
    cal.border_value = (int)c[36];
    return true;
}

static bool write_rig(const StereoRig &rig)
{
    double v[20];
    for (int i = 0; i < 9; ++i) { v[i] = rig.R1()[i]; v[9 + i] = rig.R2()[i]; }
    v[18] = rig.Baseline(); v[19] = rig.bf();
    return put("rig", v, 20);
}

static int run_pair(bool bgr)
{
    StereoRig::Calibration cal;
    if (!calibration(cal)) return 10;
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    const int ch = bgr ? 3 : 1, type = bgr ? CV_8UC3 : CV_8UC1;
    std::vector<uint8_t> a, b, c, e;
    if (!get("left", a) || !get("right", b) || !get("c", c) || !get("e", e)) return 11;
    const size_t n = (size_t)W * H * ch;
    if (a.size() != n || b.size() != n || c.size() != n || e.size() != n) return 11;

    StereoRig rig(cal);
    Frame fl, fr, fc, fe;
    fl._color = cv::Mat(H, W, type, a.data());
    fr._color = cv::Mat(H, W, type, b.data());
    if (rig.InitPair(&fl, &fr)) return 12;                         // not rectified yet: refused, nothing uploaded
    if (fl._hip_slot >= 0 || !fl._pyramid.empty()) return 12;
    // a rig that is refused: the second camera to the left of the first
    StereoRig::Calibration bad = cal;
    bad.T[0] = -bad.T[0];
    StereoRig refused(bad);
    if (refused.Rectify() || refused.Rectified() || refused.InitPair(&fl, &fr)) return 13;
    if (!rig.Rectify() || !rig.Rectified() || !write_rig(rig)) return 14;
    if (rig.InitPair(&fl, nullptr) || rig.InitPair(&fl, &fl)) return 15;
    if (!rig.InitPair(&fl, &fr)) return 16;
    if (fl._pyramid.size() != 3 || fr._pyramid.size() != 3 || fl._hip_slot < 0 || fr._hip_slot < 0) return 17;
    hip::Runtime &rt = hip::Runtime::Get();
    if (rt.RigCamera(&fl) != 0 || rt.RigCamera(&fr) != 1 || rt.RigCamera(&fc) != -1) return 18;
    if (!take(&fl, "l_before") || !take(&fr, "r_before")) return 19;
    if (!put("l_mirror_l0", fl._pyramid[0].data, (size_t)W * H)) return 19;
    if (fr._pyramid[0].empty()) return 20;                         // the mirror of level 0 is fetched ...
    fr._color = cv::Mat();                                         // ... and the picture released: the frame can only come back from the mirror
    // two plain frames take both slots: the rig does not touch them
    fc._color = cv::Mat(H, W, type, c.data());
    fc.InitFrame();
    fe._color = cv::Mat(H, W, type, e.data());
    fe.InitFrame();
    if (fl._hip_slot >= 0 || fr._hip_slot >= 0 || fc._hip_slot < 0 || fe._hip_slot < 0) return 21;      // both evicted
    if (!take(&fc, "c", 1) || !take(&fe, "e", 1)) return 22;
    if (!take(&fl, "l_after")) return 23;                          // from _color: uploaded and rectified again
    if (!take(&fr, "r_after")) return 24;                          // from the _pyramid[0] mirror: already rectified, uploaded as it is
    if (fl._hip_slot < 0 || fr._hip_slot < 0) return 25;
    // a plain InitFrame ends the membership
    fl.InitFrame();
    if (rt.RigCamera(&fl) != -1 || !take(&fl, "l_plain", 1)) return 26;
    return 0;
}

static bool put_features(const Frame &f, const std::string &side)
{
    const size_t n = f._features.size();
    std::vector<double> px(2 * n); std::vector<int32_t> level(n); std::vector<uint8_t> desc(32 * n);
    for (size_t i = 0; i < n; ++i) {
        const Feature *ft = f._features[i];
        px[2 * i] = ft->_pixel[0]; px[2 * i + 1] = ft->_pixel[1]; level[i] = ft->_level;
        memcpy(&desc[32 * i], ft->_desc.data, 32);
    }
    return put(side + "_px", px.data(), px.size()) && put(side + "_level", level.data(), n) && put(side + "_desc", desc.data(), desc.size());
}

static int run_stereo()
{
    StereoRig::Calibration cal;
    if (!calibration(cal)) return 30;
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    std::vector<uint8_t> a, b;
    if (!get("raw_left", a) || !get("raw_right", b) || a.size() != (size_t)W * H || b.size() != a.size()) return 31;
    StereoRig rig(cal);
    if (!rig.Rectify() || !write_rig(rig)) return 32;
    Frame fl, fr;
    fl._color = cv::Mat(H, W, CV_8UC1, a.data());
    fr._color = cv::Mat(H, W, CV_8UC1, b.data());
    if (!rig.InitPair(&fl, &fr)) return 33;
    if (!take(&fl, "sl", 3) || !take(&fr, "sr", 3)) return 34;
    FeatureDetector det;
    det.LoadParams();
    det.Detect(&fl);
    det.Detect(&fr);
    if (fl._features.empty() || fr._features.empty() || !put_features(fl, "l") || !put_features(fr, "r")) return 35;
    StereoMatcher::Options opt;
    opt._baseline = rig.Baseline();
    StereoMatcher sm(opt);
    std::vector<double> u_right;
    const int n = (int)fl._features.size();
    const int set = sm.ComputeStereoMatches(&fl, &fr, &u_right);
    if ((int)u_right.size() != n || (int)sm.GetStatus().size() != n) return 36;
    std::vector<double> depth((size_t)n);
    for (int i = 0; i < n; ++i) depth[(size_t)i] = fl._features[(size_t)i]->_depth;
    std::vector<int32_t> status(sm.GetStatus().begin(), sm.GetStatus().end());
    const int32_t count = set;
    if (!put("depth", depth.data(), depth.size()) || !put("u_right", u_right.data(), u_right.size()) || !put("status", status.data(), status.size()) ||
        !put("count", &count, 1)) return 37;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: rect_surface <dir> bgr|gray|stereo\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = strcmp(argv[2], "stereo") == 0 ? run_stereo() : run_pair(strcmp(argv[2], "bgr") == 0);
    } catch (const std::exception &ex) {
        fprintf(stderr, "rect_surface: %s\n", ex.what());
        return 4;
    }
    printf("rect_surface %s: %d\n", argv[2], rc);
    return rc;
}
