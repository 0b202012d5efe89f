// ygz::StereoMapper (include/ygz/Algorithm/StereoMapper.h), a stand-alone program for tests/test_smap_surface_build.py and
// tests/test_gpu_smap_surface.py: written against include/ygz only.
//   smap_surface run|seq <dir> <keyframe> <cov,cov,...>
// reads a synthetic stereo map: kf_poses.bin (float64 [K][7]) and the features in file order: ft_kf.bin, ft_level.bin, ft_node.bin (int32 [M]),
// ft_px.bin (float64 [M][2]), ft_depth.bin, ft_ur.bin (float64 [M]: Feature::_depth and the keyframe's u_right entry), ft_desc.bin (uint8
// [M][32]), ft_has.bin (uint8 [M]: 1, the feature already has a map point of its own; 2, it has one that is bad).  Keyframe k gets its features in file order, each in the
// FeatureVector node ft_node; keyframe <keyframe> gets the listed covisible keyframes.  The baseline is 0.1 m, the pyramid has 4 levels, the
// camera is fx = fy = 500, cx = 320, cy = 240 (camera.bin has what the program used).  Scenarios, each on a fresh copy of the map:
//   kp    CreateKeyframePoints(<keyframe>)
//   np    CreateNewMapPoints(<keyframe>), then (ba) BundleAdjuster::LocalBundleAdjustment(<keyframe>) on the grown map, the keyframe's covisible
//         list cut to the neighbours that were matched
//   bad   both calls with _chi2_mono = -1: the device calls are refused
// Written to <dir> per scenario <s>: <s>_ret (int32: return value, GetCreated().size()); the map afterwards, keyframes in order, features in
// order: <s>_feat (int64: the map point's id or -1), <s>_fdepth (float64), <s>_fbad (uint8); the map points, the old ones then the created
// ones: <s>_mp (int64 [..][6]: id, _first_seen, _last_seen, _cnt_visible, _cnt_found, _bad), <s>_mp_pos (float64 [..][3]), <s>_mp_obs (int64
// [..][3]: point id, keyframe id, feature index, per point in key order); the map before as before_*.  For np also np_codes, np_methods,
// np_pair_nb (int32 [N]), np_pairs (int32 [N][2]), np_nb_ids (int64: the matched neighbours' keyframe ids), np_created (int64: ids in creation
// order).  For ba: ba_ret (int32: return value, GetOutlierCount, rounds_run, points_left_out) and the exported problem ba_kf_ids, ba_point_ids
// (int64), ba_poses, ba_points, ba_obs, ba_fixed, ba_kind, ba_edge_pose, ba_edge_point, ba_level, ba_outlier, ba_status.
// `seq` takes a rendered rectified pair sequence instead: seq_left.bin, seq_right.bin (uint8 [K][480][640], gray), kf_poses.bin and vocab.bin (a
// DBoW3 vocabulary).  Every left and right picture goes through InitFrame, FeatureDetector::Detect and ComputeAngleAndDescriptor, the left
// features get Feature::_depth and the keyframe its u_right from StereoMatcher::ComputeStereoMatches (baseline 0.1), the left frame its
// FeatureVector from Frame::ComputeBoW; what these calls left in the frames is written out as the ft_*.bin files above (ft_node -1: the feature
// is in no node; ft_has all 0) and the same scenarios run on it, with the configuration's default camera and pyramid.
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
    std::vector<double> kf_poses, px, depth, ur;
    std::vector<int32_t> kf, level, node;
    std::vector<uint8_t> desc, has;
};

struct World {
    std::vector<Frame *> kfs;
    std::vector<MapPoint *> mps;                    // the old ones
    std::vector<std::vector<double>> u_right;
    ~World() { for (Frame *k : kfs) delete k; }
};

static void build(World &w, const Files &in, int keyframe, const std::vector<int> &cov)
{
    Memory::Clean();
    const size_t K = in.kf_poses.size() / 7;
    for (size_t k = 0; k < K; ++k) {
        Frame *kf = new Frame;
        Memory::RegisterKeyFrame(kf);
        kf->_id = kf->_keyframe_id;
        kf->_TCW = SE3::from7(&in.kf_poses[7 * k]);
        w.kfs.push_back(kf);
    }
    w.u_right.assign(K, std::vector<double>());
    for (size_t i = 0; i < in.kf.size(); ++i) {
        Frame *kf = w.kfs[in.kf[i]];
        Feature *f = new Feature(Vector2d(in.px[2 * i], in.px[2 * i + 1]), in.level[i]);
        f->_frame = kf; f->_depth = in.depth[i];
        memcpy(f->_desc.data, &in.desc[32 * i], 32);
        if (in.node[i] >= 0) kf->_feature_vec[(unsigned int)in.node[i]].push_back((unsigned int)kf->_features.size());
        if (in.has[i]) {
            MapPoint *mp = Memory::CreateMapPoint();
            mp->_pos_world = kf->_TCW.inverse() * Vector3d(0, 0, 5.0);
            mp->_obs[kf->_keyframe_id] = f;
            mp->_first_seen = mp->_last_seen = kf->_keyframe_id; mp->_cnt_visible = mp->_cnt_found = 1;
            mp->_bad = in.has[i] == 2;
            f->_mappoint = mp;
            w.mps.push_back(mp);
        }
        kf->_features.push_back(f);
        w.u_right[in.kf[i]].push_back(in.ur[i]);
    }
    for (int c : cov) { w.kfs[keyframe]->_cov_keyframes.push_back(w.kfs[c]); w.kfs[keyframe]->_cov_weights.push_back(100); }
}

static bool dump_map(const std::string &s, const World &w, const std::vector<MapPoint *> &created)
{
    std::vector<int64_t> feat, mp, obs;
    std::vector<double> fdepth, pos;
    std::vector<uint8_t> fbad;
    for (const Frame *kf : w.kfs)
        for (const Feature *f : kf->_features) {
            feat.push_back(f->_mappoint ? (int64_t)f->_mappoint->_id : -1);
            fdepth.push_back(f->_depth); fbad.push_back(f->_bad ? 1 : 0);
        }
    std::vector<MapPoint *> all = w.mps;
    all.insert(all.end(), created.begin(), created.end());
    for (const MapPoint *m : all) {
        mp.push_back((int64_t)m->_id); mp.push_back((int64_t)m->_first_seen); mp.push_back((int64_t)m->_last_seen);
        mp.push_back(m->_cnt_visible); mp.push_back(m->_cnt_found); mp.push_back(m->_bad ? 1 : 0);
        for (int k = 0; k < 3; ++k) pos.push_back(m->_pos_world[k]);
        for (const auto &ob : m->_obs) {
            const Frame *kf = ob.second->_frame;
            int64_t ix = -1;
            for (size_t i = 0; i < kf->_features.size(); ++i) if (kf->_features[i] == ob.second) ix = (int64_t)i;
            obs.push_back((int64_t)m->_id); obs.push_back((int64_t)ob.first); obs.push_back(ix);
        }
    }
    return put(s + "_feat", feat) && put(s + "_fdepth", fdepth) && put(s + "_fbad", fbad) && put(s + "_mp", mp) && put(s + "_mp_pos", pos) &&
           put(s + "_mp_obs", obs);
}

static bool dump_ba(const BundleAdjuster &ba, bool ret)
{
    const std::string s = "ba";
    const BundleAdjuster::Problem &g = ba.GetProblem();
    const BundleAdjuster::Result &r = ba.GetResult();
    std::vector<int32_t> status;
    for (int k = 0; k < 4; ++k) status.push_back(r._rounds[k]._status);
    const std::vector<int32_t> rets = { ret ? 1 : 0, ba.GetOutlierCount(), r._rounds_run, g.points_left_out };
    return put(s + "_ret", rets) && put(s + "_kf_ids", std::vector<int64_t>(g.keyframe_ids.begin(), g.keyframe_ids.end())) &&
           put(s + "_point_ids", std::vector<int64_t>(g.point_ids.begin(), g.point_ids.end())) && put(s + "_poses", g.poses) &&
           put(s + "_points", g.points) && put(s + "_obs", g.obs) && put(s + "_fixed", g.fixed) && put(s + "_kind", g.kind) &&
           put(s + "_edge_pose", g.edge_pose) && put(s + "_edge_point", g.edge_point) && put(s + "_level", g.level) &&
           put(s + "_outlier", g.outlier) && put(s + "_status", status);
}

static int scenarios(const Files &in, int keyframe, const std::vector<int> &cov, const PinholeCamera &cam);

static int run(int keyframe, const std::vector<int> &cov)
{
    Config::Set("image.width", "640"); Config::Set("image.height", "480"); Config::Set("frame.pyramid", "4");
    Config::Set("camera.fx", "500"); Config::Set("camera.fy", "500"); Config::Set("camera.cx", "320"); Config::Set("camera.cy", "240");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    Files in;
    if (!get("kf_poses", in.kf_poses) || !get("ft_kf", in.kf) || !get("ft_level", in.level) || !get("ft_node", in.node) || !get("ft_px", in.px) ||
        !get("ft_depth", in.depth) || !get("ft_ur", in.ur) || !get("ft_desc", in.desc) || !get("ft_has", in.has))
        return 10;
    return scenarios(in, keyframe, cov, cam);
}

// the map's arrays from rendered pairs: what the detector, the stereo matcher and ComputeBoW leave in the frames
static int run_seq(int keyframe, const std::vector<int> &cov)
{
    const int W = 640, H = 480;
    Config::Set("image.width", "640"); Config::Set("image.height", "480");
    PinholeCamera cam;
    Frame::SetCamera(&cam);
    std::vector<uint8_t> left, right, vocab;
    Files in;
    if (!get("seq_left", left) || !get("seq_right", right) || !get("vocab", vocab) || !get("kf_poses", in.kf_poses)) return 20;
    const size_t K = in.kf_poses.size() / 7, fb = (size_t)W * H;
    if (K < 2 || left.size() != K * fb || right.size() != left.size()) return 21;
    ORBVocabulary voc;
    if (!voc.loadFromMemory(vocab.data(), vocab.size())) return 22;
    Frame::SetORBVocabulary(&voc);
    FeatureDetector det;
    det.LoadParams();
    StereoMatcher::Options opt;
    opt._baseline = 0.1;
    StereoMatcher matcher(opt);
    for (size_t k = 0; k < K; ++k) {
        Frame fl, fr;
        fl._color = cv::Mat(H, W, CV_8UC1, left.data() + k * fb);
        fr._color = cv::Mat(H, W, CV_8UC1, right.data() + k * fb);
        fl.InitFrame(); fr.InitFrame();
        fl._TCW = SE3::from7(&in.kf_poses[7 * k]); fr._TCW = fl._TCW;
        det.Detect(&fl); det.ComputeAngleAndDescriptor(&fl);
        det.Detect(&fr); det.ComputeAngleAndDescriptor(&fr);
        std::vector<double> u_right;
        const int set = matcher.ComputeStereoMatches(&fl, &fr, &u_right);
        if (fl._features.empty() || u_right.size() != fl._features.size() || set <= 0) return 23;
        fl.ComputeBoW();
        std::vector<int32_t> node(fl._features.size(), -1);
        for (const auto &kv : fl._feature_vec) for (unsigned int idx : kv.second) if (idx < node.size()) node[idx] = (int32_t)kv.first;
        for (size_t i = 0; i < fl._features.size(); ++i) {
            const Feature *f = fl._features[i];
            in.kf.push_back((int32_t)k); in.level.push_back(f->_level); in.node.push_back(node[i]);
            in.px.push_back(f->_pixel[0]); in.px.push_back(f->_pixel[1]); in.depth.push_back(f->_depth); in.ur.push_back(u_right[i]);
            in.desc.insert(in.desc.end(), f->_desc.data, f->_desc.data + 32);
            in.has.push_back(0);
        }
    }
    Frame::SetORBVocabulary(nullptr);
    if (!put("ft_kf", in.kf) || !put("ft_level", in.level) || !put("ft_node", in.node) || !put("ft_px", in.px) || !put("ft_depth", in.depth) ||
        !put("ft_ur", in.ur) || !put("ft_desc", in.desc) || !put("ft_has", in.has))
        return 24;
    return scenarios(in, keyframe, cov, cam);
}

static int scenarios(const Files &in, int keyframe, const std::vector<int> &cov, const PinholeCamera &cam)
{
    const std::vector<double> k4 = { (double)cam.fx(), (double)cam.fy(), (double)cam.cx(), (double)cam.cy() };
    if (!put("camera", k4)) return 10;
    const std::vector<MapPoint *> none;
    {   // kp
        World w;
        build(w, in, keyframe, cov);
        if (!dump_map("before", w, none)) return 11;
        StereoMapper sm;
        if (sm.CreateKeyframePoints(nullptr) != 0 || sm.CreateNewMapPoints(nullptr) != 0) return 12;
        const int ret = sm.CreateKeyframePoints(w.kfs[keyframe]);
        const std::vector<int32_t> rets = { ret, (int32_t)sm.GetCreated().size() };
        if (!put("kp_ret", rets) || !dump_map("kp", w, sm.GetCreated())) return 13;
    }
    {   // np, ba
        World w;
        build(w, in, keyframe, cov);
        StereoMapper sm;
        for (size_t k = 0; k < w.kfs.size(); ++k) sm.SetURight(w.kfs[k], w.u_right[k]);
        const int ret = sm.CreateNewMapPoints(w.kfs[keyframe]);
        const std::vector<int32_t> rets = { ret, (int32_t)sm.GetCreated().size() };
        std::vector<int32_t> pairs;
        for (const auto &p : sm.GetPairs()) { pairs.push_back(p.first); pairs.push_back(p.second); }
        std::vector<int64_t> nb, created;
        for (const Frame *f : sm.GetNeighbours()) nb.push_back((int64_t)f->_keyframe_id);
        for (const MapPoint *m : sm.GetCreated()) created.push_back((int64_t)m->_id);
        if (!put("np_ret", rets) || !dump_map("np", w, sm.GetCreated()) || !put("np_codes", sm.GetCodes()) || !put("np_methods", sm.GetMethods()) ||
            !put("np_pair_nb", sm.GetPairNeighbour()) || !put("np_pairs", pairs) || !put("np_nb_ids", nb) || !put("np_created", created))
            return 14;
        // the local window of the adjustment: the neighbours that were matched (a skipped one shares no point with the keyframe)
        w.kfs[keyframe]->_cov_keyframes = sm.GetNeighbours();
        w.kfs[keyframe]->_cov_weights.assign(sm.GetNeighbours().size(), 100);
        BundleAdjuster ba;
        for (size_t k = 0; k < w.kfs.size(); ++k) ba.SetURight(w.kfs[k], w.u_right[k]);
        const bool ok = ba.LocalBundleAdjustment(w.kfs[keyframe]);
        if (!dump_ba(ba, ok)) return 15;
    }
    {   // bad
        World w;
        build(w, in, keyframe, cov);
        StereoMapper sm;
        for (size_t k = 0; k < w.kfs.size(); ++k) sm.SetURight(w.kfs[k], w.u_right[k]);
        sm._options._chi2_mono = -1.0;
        const int r1 = sm.CreateKeyframePoints(w.kfs[keyframe]), c1 = (int)sm.GetCreated().size();
        const int r2 = sm.CreateNewMapPoints(w.kfs[keyframe]), c2 = (int)sm.GetCreated().size();
        const std::vector<int32_t> rets = { r1, c1, r2, c2, (int32_t)sm.GetCodes().size() };
        if (!put("bad_ret", rets) || !dump_map("bad", w, none)) return 16;
    }
    Memory::Clean();
    return 0;
}

int main(int argc, char **argv)
{
    if (!(argc == 5 && (!strcmp(argv[1], "run") || !strcmp(argv[1], "seq")))) { fprintf(stderr, "usage: smap_surface run|seq <dir> <keyframe> <cov,cov,...>\n"); return 2; }
    g_dir = argv[2];
    std::vector<int> cov;
    for (char *t = strtok(argv[4], ","); t; t = strtok(nullptr, ",")) cov.push_back(atoi(t));
    int rc = 3;
    try {
        rc = !strcmp(argv[1], "seq") ? run_seq(atoi(argv[3]), cov) : run(atoi(argv[3]), cov);
    } catch (const std::exception &ex) {
        fprintf(stderr, "smap_surface: %s\n", ex.what());
        return 4;
    }
    printf("smap_surface: %s\n", rc == 0 ? "ok" : "failed");
    return rc;
}
