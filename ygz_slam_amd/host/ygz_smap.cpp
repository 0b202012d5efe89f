// ygz::StereoMapper (include/ygz/Algorithm/StereoMapper.h): nothing in the reference.  ORB-SLAM2's two map-point creation paths for a stereo
// or RGB-D keyframe as synchronous calls: the keyframe's features (or its matches with the covisible neighbours, all neighbours together) go
// through ONE device call (ygz_slam_amd/csrc/smap.hip), and the map is written from its result.  Every order goes by index.  Not part of it:
// covisibility upkeep, distinctive descriptors; SearchInNeighbors and MapPointCulling are in ygz_lfuse.cpp.
// Error conventions of the other surfaces: a failed call logs and returns 0 and leaves the map unchanged, only a missing device throws.
#include "ygz/Algorithm/StereoMapper.h"
#include "ygz/Algorithm/Matcher.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"

namespace ygz {

namespace {
bool has_good_point(const Feature *f) { return f && f->_mappoint != nullptr && !f->_mappoint->_bad; }

// a feature about to receive a new point leaves the observations of the (bad) point it still names
void detach(Feature *f)
{
    MapPoint *old = f->_mappoint;
    if (!old) return;
    for (auto it = old->_obs.begin(); it != old->_obs.end();) { if (it->second == f) it = old->_obs.erase(it); else ++it; }
    f->_mappoint = nullptr;
}
}

void StereoMapper::SetURight(const Frame *kf, const std::vector<double> &u_right) { if (kf) _u_right[kf->_keyframe_id] = u_right; }
void StereoMapper::ClearURight(const Frame *kf) { if (kf) _u_right.erase(kf->_keyframe_id); }
void StereoMapper::Clear() { _u_right.clear(); }

double StereoMapper::URight(const Frame *kf, size_t index) const
{
    auto u = _u_right.find(kf->_keyframe_id);
    return u != _u_right.end() && index < u->second.size() ? u->second[index] : -1.0;
}

int StereoMapper::CreateKeyframePoints(Frame *kf)
{
    _codes.clear(); _methods.clear(); _pair_neighbour.clear(); _pairs.clear(); _neighbours.clear(); _created.clear();
    const PinholeCamera *cam = Frame::GetCamera();
    if (!kf || !cam) { LOG(ERROR) << "StereoMapper::CreateKeyframePoints: no keyframe or no camera" << endl; return 0; }
    const size_t n = kf->_features.size();
    std::vector<double> px(2 * n + 2), depth(n + 1), pos(3 * n + 3);
    std::vector<uint8_t> has(n + 1), selected(n + 1);
    std::vector<int32_t> rank(n + 1);
    for (size_t i = 0; i < n; ++i) {
        const Feature *f = kf->_features[i];
        if (!f) { LOG(ERROR) << "StereoMapper::CreateKeyframePoints: a null feature" << endl; return 0; }
        px[2 * i] = f->_pixel[0]; px[2 * i + 1] = f->_pixel[1]; depth[i] = f->_depth; has[i] = has_good_point(f) ? 1 : 0;
    }
    ygz_smap_params p;
    ygz_hip_default_smap_params(&p);
    p.baseline = _options._baseline; p.chi2_mono = _options._chi2_mono; p.chi2_stereo = _options._chi2_stereo;
    p.cos_parallax_max = _options._cos_parallax_max; p.th_depth = _options._th_depth; p.min_close = _options._min_close;
    const double K4[4] = { (double)cam->fx(), (double)cam->fy(), (double)cam->cx(), (double)cam->cy() };
    double T[7];
    kf->_TCW.to7(T);
    int n_selected = 0;
    if (!hip::check(ygz_hip_stereo_keyframe_points(hip::Runtime::Get().ctx(), T, (int)n, px.data(), depth.data(), has.data(), K4, &p, rank.data(),
                                                   selected.data(), pos.data(), nullptr, nullptr, &n_selected), "stereo_keyframe_points"))
        return 0;
    for (size_t i = 0; i < n; ++i) {
        if (!selected[i]) continue;
        Feature *f = kf->_features[i];
        detach(f);
        MapPoint *mp = Memory::CreateMapPoint();
        mp->_first_seen = mp->_last_seen = kf->_keyframe_id;
        mp->_obs[kf->_keyframe_id] = f;
        mp->_cnt_visible = 1; mp->_cnt_found = 1;
        mp->_pos_world = Vector3d(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
        f->_mappoint = mp;
        f->_bad = false;
        _created.push_back(mp);
        _recent.push_back(mp);
    }
    return (int)_created.size();
}

int StereoMapper::CreateNewMapPoints(Frame *kf)
{
    _codes.clear(); _methods.clear(); _pair_neighbour.clear(); _pairs.clear(); _neighbours.clear(); _created.clear();
    const PinholeCamera *cam = Frame::GetCamera();
    if (!kf || kf->_bad || !cam) { LOG(ERROR) << "StereoMapper::CreateNewMapPoints: no keyframe or no camera" << endl; return 0; }
    const Vector3d cam_current = kf->GetCamCenter();
    struct Arrays { std::vector<double> px1, px2, ur1, ur2, d1, d2; std::vector<int32_t> l1, l2; };
    std::vector<Arrays> arrays;
    std::vector<ygz_smap_problem> problems;
    int taken = 0;
    for (Frame *f2 : kf->_cov_keyframes) {
        if (taken >= _options._neighbours) break;
        if (!f2 || f2->_bad) continue;
        ++taken;
        if ((cam_current - f2->GetCamCenter()).norm() < _options._baseline) continue;       // ORB-SLAM2's stereo rule
        // LocalMapping.cpp:401-405: E12 = t12^ R12 of T12 = T_current * T_neighbour^-1
        const SE3 T12 = kf->_TCW * f2->_TCW.inverse();
        const Matrix3d E12 = SO3::hat(T12.translation()) * T12.rotation_matrix();
        vector<pair<int, int>> matched;
        Matcher matcher;
        matcher.SearchForTriangulation(kf, f2, E12, matched);
        Arrays a;
        const int nb = (int)_neighbours.size();
        for (const auto &m : matched) {
            const Feature *fa = kf->_features[m.first], *fb = f2->_features[m.second];
            if (!fa || !fb || has_good_point(fa) || has_good_point(fb)) continue;
            a.px1.push_back(fa->_pixel[0]); a.px1.push_back(fa->_pixel[1]); a.px2.push_back(fb->_pixel[0]); a.px2.push_back(fb->_pixel[1]);
            a.ur1.push_back(URight(kf, (size_t)m.first)); a.ur2.push_back(URight(f2, (size_t)m.second));
            a.d1.push_back(fa->_depth); a.d2.push_back(fb->_depth);
            a.l1.push_back(fa->_level); a.l2.push_back(fb->_level);
            _pairs.push_back(m); _pair_neighbour.push_back(nb);
        }
        _neighbours.push_back(f2);
        arrays.push_back(std::move(a));
    }
    if (_neighbours.empty()) return 0;
    problems.resize(_neighbours.size());
    for (size_t q = 0; q < _neighbours.size(); ++q) {
        ygz_smap_problem &pb = problems[q];
        const Arrays &a = arrays[q];
        kf->_TCW.to7(pb.T1); _neighbours[q]->_TCW.to7(pb.T2);
        pb.px1 = a.px1.data(); pb.px2 = a.px2.data(); pb.ur1 = a.ur1.data(); pb.ur2 = a.ur2.data(); pb.depth1 = a.d1.data(); pb.depth2 = a.d2.data();
        pb.level1 = a.l1.data(); pb.level2 = a.l2.data(); pb.n = (int)a.ur1.size();
    }
    ygz_smap_params p;
    ygz_hip_default_smap_params(&p);
    p.baseline = _options._baseline; p.chi2_mono = _options._chi2_mono; p.chi2_stereo = _options._chi2_stereo;
    p.cos_parallax_max = _options._cos_parallax_max; p.th_depth = _options._th_depth; p.min_close = _options._min_close;
    const double K4[4] = { (double)cam->fx(), (double)cam->fy(), (double)cam->cx(), (double)cam->cy() };
    const size_t N = _pairs.size();
    _codes.assign(N + 1, 0); _methods.assign(N + 1, 0);
    std::vector<double> pos(3 * N + 3);
    const bool ok = hip::check(ygz_hip_stereo_create_map_points(hip::Runtime::Get().ctx(), (int)problems.size(), problems.data(), K4, &p, _codes.data(),
                                                                _methods.data(), pos.data(), nullptr), "stereo_create_map_points");
    _codes.resize(ok ? N : 0); _methods.resize(ok ? N : 0);
    if (!ok) { _pairs.clear(); _pair_neighbour.clear(); _neighbours.clear(); return 0; }
    // the walk: neighbour order, then pair order (the order of the call's pairs); a feature takes at most one point
    for (size_t i = 0; i < N; ++i) {
        if (_codes[i] != 0) continue;
        Frame *f2 = _neighbours[_pair_neighbour[i]];
        Feature *fa = kf->_features[_pairs[i].first], *fb = f2->_features[_pairs[i].second];
        if (has_good_point(fa) || has_good_point(fb)) continue;
        detach(fa); detach(fb);
        MapPoint *mp = Memory::CreateMapPoint();                         // LocalMapping.cpp:469-485
        mp->_first_seen = mp->_last_seen = kf->_keyframe_id;
        mp->_obs[kf->_keyframe_id] = fa;
        mp->_obs[f2->_keyframe_id] = fb;
        mp->_cnt_visible = 2; mp->_cnt_found = 2;
        mp->_pos_world = Vector3d(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
        fa->_mappoint = mp; fb->_mappoint = mp;
        if (URight(kf, (size_t)_pairs[i].first) < 0) fa->_depth = (kf->_TCW * mp->_pos_world)[2];
        if (URight(f2, (size_t)_pairs[i].second) < 0) fb->_depth = (f2->_TCW * mp->_pos_world)[2];
        fa->_bad = fb->_bad = false;
        _created.push_back(mp);
        _recent.push_back(mp);
    }
    return (int)_created.size();
}

}  // namespace ygz
