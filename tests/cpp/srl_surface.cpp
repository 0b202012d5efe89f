// ygz::StereoRelocalizer (include/ygz/Algorithm/StereoRelocalizer.h), a stand-alone program for tests/test_srl_surface_build.py and
// tests/test_gpu_srl_surface.py: written against include/ygz only.
//   srl_surface <dir>
// reads a small stereo map: a vocabulary (vocab, DBoW3's binary format), three keyframes and three lost frames, each with a QVGA gray picture
// k<j>_img / f<k>_img (uint8 [240][320]), its features _px (float64 [n][2]), _level (int32 [n]), _angle, _depth (float64 [n]; <= 0: none) and
// its pose _pose (float64 [7]; a frame's is what a lost frame happens to hold); a keyframe's features also have k<j>_mp (int32 [n]: the map
// point or -1); the map points mp_pos (float64 [P][3]).  The candidates of frame 0 are keyframes 2, 0, 1 in that order, those of frame 1 are
// keyframes 1, 0, those of frame 2 keyframes 0, 1.  A feature's _desc is what the device describes at its pixel, so that the host-array route
// sees the descriptors the resident route computes.  Scenarios, each on a fresh copy of the map:
//   old     per frame and per candidate in order: every _mappoint cleared, Matcher::SearchByBoW(keyframe, frame) with checkOrientation off,
//           th_low 50 and knnRatio 0.75, the claim of ygz_reloc.cpp (a frame feature goes to the first keyframe feature with a good point
//           that names it), the associations put in the order of the frame's features; with at least 15 of them ygz_hip_pnp_ransac with the
//           default parameters; with its success the inliers' _mappoint, _TCW the PnP pose, PoseOptimizer::Optimize with
//           PoseOptimizer::URightFromDepth (the points' _cnt_found saved and restored); the first candidate with at least 50 features that
//           are not _bad wins: a _bad feature loses its _mappoint and _ref_keyframe is the keyframe.  A candidate that fails, and a frame no
//           candidate of which wins, leave the frame as it was
//   batch   ONE StereoRelocalizer::Relocalize over the three frames, _check_orientation off
//   single  StereoRelocalizer::Relocalize of frame 1 alone
// Written to <dir>: per scenario <s>: <s>_pose (float64 [3][7]), <s>_feat<k> (int32 per feature: the map point's index or -1), <s>_bad<k> (uint8),
// <s>_depth<k> (float64), <s>_found (int32 [P]: _cnt_found), <s>_ref (int32 [3]: the keyframe _ref_keyframe is, 3 for none of them), <s>_ret
// (int32: old: per frame the winner's place in its list, then per candidate the associations, the PnP inliers, the features kept (-1 where the
// candidate did not get that far); batch, single: the return value, then per frame the winner, then per candidate status, matches, PnP
// inliers, final inliers); untouched (int32: 1 when no scenario made a map point or a keyframe).
#include "ygz/Basic.h"
#include "ygz/Algorithm.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

using namespace ygz;

static std::string g_dir;
static const int W = 320, H = 240, NF = 3, NK = 3;

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
    std::vector<int32_t> found, ref;
    for (int k = 0; k < NF; ++k) {
        const Frame *f = w.frames[(size_t)k];
        f->_TCW.to7(&pose[7 * (size_t)k]);
        ref.push_back((int32_t)(std::find(w.kfs.begin(), w.kfs.end(), f->_ref_keyframe) - w.kfs.begin()));      // NK: none of them
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
    return put(s + "_pose", pose) && put(s + "_found", found) && put(s + "_ref", ref) && put(s + "_ret", ret);
}

static std::vector<std::vector<Frame *>> candidates(const World &w)
{
    return { { w.kfs[2], w.kfs[0], w.kfs[1] }, { w.kfs[1], w.kfs[0] }, { w.kfs[0], w.kfs[1] } };
}

static std::vector<int32_t> flat(int ret, const std::vector<StereoRelocalizer::Result> &res)
{
    std::vector<int32_t> o(1, ret);
    for (const StereoRelocalizer::Result &r : res) {
        o.push_back(r.winner);
        for (size_t q = 0; q < r.status.size(); ++q) o.insert(o.end(), { r.status[q], r.matches[q], r.pnp_inliers[q], r.final_inliers[q] });
    }
    return o;
}

struct Saved { SE3 T; Frame *ref; std::vector<MapPoint *> mp; std::vector<char> bad; std::vector<double> depth; };

static Saved save(const Frame *f)
{
    Saved s;
    s.T = f->_TCW; s.ref = f->_ref_keyframe;
    for (const Feature *ft : f->_features) { s.mp.push_back(ft->_mappoint); s.bad.push_back(ft->_bad ? 1 : 0); s.depth.push_back(ft->_depth); }
    return s;
}

static void restore(Frame *f, const Saved &s)
{
    f->_TCW = s.T; f->_ref_keyframe = s.ref;
    for (size_t j = 0; j < f->_features.size(); ++j) {
        Feature *ft = f->_features[j];
        ft->_mappoint = s.mp[j]; ft->_bad = s.bad[j] != 0; ft->_depth = s.depth[j];
    }
}

// the host route for one frame: the winner's place in `cands` or -1; ret gets three numbers per candidate
static int old_route(Frame *cur, const std::vector<Frame *> &cands, Matcher &matcher, PoseOptimizer &opt, std::vector<int32_t> &ret)
{
    const Saved before = save(cur);
    const Matrix3d K = Frame::GetCamera()->GetCameraMatrix();
    const double K4[4] = { K(0, 0), K(1, 1), K(0, 2), K(1, 2) };
    int winner = -1;
    for (size_t q = 0; q < cands.size(); ++q) {
        Frame *kf = cands[q];
        int32_t n_pnp = -1, n_kept = -1;
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
        std::sort(got.begin(), got.end(), [](const std::pair<int, MapPoint *> &a, const std::pair<int, MapPoint *> &b) { return a.first < b.first; });
        bool won = false;
        if ((int)got.size() >= 15) {
            std::vector<double> pw, px;
            for (const auto &g : got) {
                for (int e = 0; e < 3; ++e) pw.push_back(g.second->_pos_world[e]);
                px.push_back(cur->_features[(size_t)g.first]->_pixel[0]); px.push_back(cur->_features[(size_t)g.first]->_pixel[1]);
            }
            const int32_t off[2] = { 0, (int32_t)got.size() };
            ygz_pnp_params prm;
            ygz_hip_default_pnp_params(&prm);
            ygz_pnp_result res;
            std::vector<uint8_t> inl(got.size());
            if (ygz_hip_pnp_ransac(hip::Runtime::Get().ctx(), 1, off, pw.data(), px.data(), K4, &prm, &res, inl.data()) != YGZ_OK) return -2;
            n_pnp = res.n_inliers;
            if (res.success) {
                std::vector<int> found;
                for (size_t e = 0; e < got.size(); ++e)
                    if (inl[e]) { cur->_features[(size_t)got[e].first]->_mappoint = got[e].second; found.push_back(got[e].second->_cnt_found); }
                cur->_TCW = SE3::from7(res.T_cw);
                std::vector<double> ur;
                PoseOptimizer::URightFromDepth(cur, opt._options._baseline, &ur);
                opt.Optimize(cur, &ur);
                size_t at = 0;
                for (size_t e = 0; e < got.size(); ++e)
                    if (inl[e]) got[e].second->_cnt_found = found[at++];
                n_kept = 0;
                for (const Feature *ft : cur->_features) n_kept += ft->_mappoint && !ft->_bad ? 1 : 0;
                won = n_kept >= 50;
            }
        }
        ret.insert(ret.end(), { (int32_t)got.size(), n_pnp, n_kept });
        if (won && winner < 0) {
            for (Feature *ft : cur->_features) if (ft->_bad) ft->_mappoint = nullptr;
            cur->_ref_keyframe = kf;
            winner = (int)q;
            break;
        }
        restore(cur, before);
    }
    return winner;
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
    StereoRelocalizer::Options o;
    o._check_orientation = false;
    {   // old: the host-array route, frame by frame and candidate by candidate
        World w;
        if (!build(w, in)) return 11;
        const unsigned long next_id = Memory::CreateMapPoint()->_id + 1;
        Matcher matcher;
        matcher._options.th_low = 50; matcher._options.knnRatio = 0.75f; matcher._options.checkOrientation = false;
        PoseOptimizer opt;
        std::vector<int32_t> ret;
        const std::vector<std::vector<Frame *>> cands = candidates(w);
        for (int k = 0; k < NF; ++k) {
            std::vector<int32_t> per;
            const int win = old_route(w.frames[(size_t)k], cands[(size_t)k], matcher, opt, per);
            if (win < -1) return 19;
            ret.push_back(win);
            ret.insert(ret.end(), per.begin(), per.end());
        }
        if (!dump("old", w, ret)) return 12;
        untouched = untouched && Memory::GetNumberFrames() == NK && Memory::CreateMapPoint()->_id == next_id && w.mps.size() == P;
    }
    {   // batch: one call
        World w;
        if (!build(w, in)) return 13;
        const unsigned long next_id = Memory::CreateMapPoint()->_id + 1;
        StereoRelocalizer rl(o);
        std::vector<StereoRelocalizer::Result> res;
        // nothing to relocalise: nothing is written
        if (rl.Relocalize({}, {}, &res) != 0 || rl.Relocalize({ w.frames[0] }, {}, &res) != 0 ||
            rl.Relocalize({ w.frames[0], w.frames[0] }, { { w.kfs[0] }, { w.kfs[0] } }, &res) != 0 ||
            rl.Relocalize({ w.frames[0], nullptr }, { { w.kfs[0] }, { w.kfs[0] } }, &res) != 0 ||
            rl.Relocalize({ w.frames[0] }, { { nullptr } }, &res) != 0 || rl.Relocalize({ w.kfs[0] }, { { w.kfs[0] } }, &res) != 0 ||
            rl.Relocalize({ w.frames[0] }, { {} }, &res) != 0 || !res.empty())
            return 14;
        const int ret = rl.Relocalize(w.frames, candidates(w), &res);
        if (res.size() != (size_t)NF || !dump("batch", w, flat(ret, res))) return 15;
        untouched = untouched && Memory::GetNumberFrames() == NK && Memory::CreateMapPoint()->_id == next_id && w.mps.size() == P;
    }
    {   // single: frame 1 alone
        World w;
        if (!build(w, in)) return 16;
        StereoRelocalizer rl(o);
        std::vector<StereoRelocalizer::Result> res;
        const int ret = rl.Relocalize({ w.frames[1] }, { candidates(w)[1] }, &res);
        if (res.size() != 1 || !dump("single", w, flat(ret, res))) return 17;
    }
    Memory::Clean();
    Frame::SetORBVocabulary(nullptr);
    if (!put("untouched", std::vector<int32_t>(1, untouched ? 1 : 0))) return 18;
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: srl_surface <dir>\n"); return 2; }
    g_dir = argv[1];
    int rc = 3;
    try {
        rc = run();
    } catch (const std::exception &ex) {
        fprintf(stderr, "srl_surface: %s\n", ex.what());
        return 4;
    }
    printf("srl_surface: %d\n", rc);
    return rc;
}
