// ygz::StereoMapper::SearchInNeighbors / MapPointCulling (include/ygz/Algorithm/StereoMapper.h): nothing in the reference.  ORB-SLAM2's
// LocalMapping::SearchInNeighbors and MapPointCulling on this data model: the search of ORBmatcher::Fuse runs on the device, all targets of a
// direction in ONE call over ONE shared point set (ygz_hip_local_fuse_search, ygz_slam_amd/csrc/lfuse.hip), and the map is edited on the host
// from its result by a walk that re-checks every hit against the map as it is by then.  The spec is DESIGN.md section 25.  Every order goes
// by list position, _keyframe_id or index, never by address.  Error conventions of the other surfaces: a failed call logs and returns 0,
// only a missing device throws.
#include "ygz/Algorithm/StereoMapper.h"
#include "ygz/Algorithm/Matcher.h"
#include "ygz/Algorithm/LoopClosing.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include <algorithm>
#include <cstring>

namespace ygz {

namespace {
using hip::good;
Frame *frame_of(unsigned long id, const Feature *f) { return f && f->_frame ? f->_frame : Memory::GetKeyFrame(id); }

int index_in_frame(const Feature *f)
{
    if (!f || !f->_frame) return -1;
    const vector<Feature *> &fs = f->_frame->_features;
    for (size_t i = 0; i < fs.size(); ++i) if (fs[i] == f) return (int)i;
    return -1;
}

// the keypoint arrays of one target keyframe
struct Keypoints {
    std::vector<double> px, ur;
    std::vector<int32_t> level;
    std::vector<uint8_t> desc;
};
}

int StereoMapper::Observations(const MapPoint *mp) const
{
    int n = 0;
    for (const auto &ob : mp->_obs) {
        const Feature *f = ob.second;
        const int ix = index_in_frame(f);
        n += (ix >= 0 && URight(f->_frame, (size_t)ix) >= 0) ? 2 : 1;
    }
    return n;
}

// the hits of one device call, problems (targets) in order, then points by index, each against the map as it is now
int StereoMapper::Walk(const std::vector<Frame *> &targets, const Search &s, std::set<Frame *> &touched)
{
    int fused = 0;
    const size_t n = s.points.size();
    std::map<const MapPoint *, MapPoint *> into;                        // replaced in this walk -> by what (looked up, never iterated)
    auto replace = [&](MapPoint *from, MapPoint *to) {
        for (const auto &ob : from->_obs)
            if (Frame *k = frame_of(ob.first, ob.second)) touched.insert(k);
        LoopClosing::ReplaceMapPoint(from, to);
        into[from] = to;
        ++_fuse_stats.replaced; ++fused;
    };
    for (size_t k = 0; k < targets.size(); ++k) {
        Frame *kf = targets[k];
        for (size_t i = 0; i < n; ++i) {
            const int j = s.match[k * n + i];
            if (j < 0 || j >= (int)kf->_features.size()) continue;
            MapPoint *P = s.points[i];
            for (auto it = into.find(P); it != into.end(); it = into.find(P)) P = it->second;
            if (!good(P) || P->_obs.count(kf->_keyframe_id)) {
                ++_fuse_stats.conflicts;
                _fusions.push_back(Fusion{ FUSE_CONFLICT, kf->_keyframe_id, s.points[i]->_id, j, P->_id });
                continue;
            }
            Feature *f = kf->_features[j];
            MapPoint *q = f->_mappoint;
            if (!good(q)) {
                if (q)                                                  // a bad point first loses the feature from its observations
                    for (auto it = q->_obs.begin(); it != q->_obs.end();) { if (it->second == f) it = q->_obs.erase(it); else ++it; }
                P->_obs[kf->_keyframe_id] = f;
                f->_mappoint = P;
                touched.insert(kf);
                ++_fuse_stats.added; ++fused;
                _fusions.push_back(Fusion{ FUSE_ADDED, kf->_keyframe_id, s.points[i]->_id, j, P->_id });
            } else if (q == P) {
                continue;
            } else if (Observations(q) > Observations(P)) {
                _fusions.push_back(Fusion{ FUSE_REPLACED_INTO_FEATURE, kf->_keyframe_id, s.points[i]->_id, j, q->_id });
                replace(P, q);
            } else {
                _fusions.push_back(Fusion{ FUSE_REPLACED_INTO_POINT, kf->_keyframe_id, s.points[i]->_id, j, P->_id });
                replace(q, P);
            }
        }
    }
    return fused;
}

int StereoMapper::SearchInNeighbors(Frame *kf, Matcher &matcher)
{
    _fusions.clear(); _touched.clear(); _targets.clear();
    _fuse_stats = FuseStats();
    _search[0] = Search(); _search[1] = Search();
    const PinholeCamera *cam = Frame::GetCamera();
    if (!kf || kf->_bad || !cam) { LOG(ERROR) << "StereoMapper::SearchInNeighbors: no keyframe or no camera" << endl; return 0; }

    // 1. the targets: ORB-SLAM2's interleaved walk
    std::vector<Frame *> targets;
    auto is_target = [&](const Frame *f) { return std::find(targets.begin(), targets.end(), f) != targets.end(); };
    int taken = 0;
    for (Frame *n1 : kf->_cov_keyframes) {
        if (taken >= _options._neighbours) break;
        if (!n1 || n1->_bad) continue;
        ++taken;
        if (n1 != kf && !is_target(n1)) targets.push_back(n1);
        int second = 0;
        for (Frame *n2 : n1->_cov_keyframes) {
            if (second >= _options._second_neighbours) break;
            if (!n2 || n2->_bad || n2 == kf || is_target(n2)) continue;
            ++second;
            targets.push_back(n2);
        }
    }
    if (targets.size() > (size_t)YGZ_LFUSE_MAX_PROBLEMS) {
        _fuse_stats.targets_dropped = (int)targets.size() - YGZ_LFUSE_MAX_PROBLEMS;
        targets.resize(YGZ_LFUSE_MAX_PROBLEMS);
    }
    _fuse_stats.targets = (int)targets.size();
    if (targets.empty()) return 0;
    ygz_hip_ctx *ctx = hip::Runtime::Get().ctx();
    // what would refuse the reverse call is refused here, before the map is touched
    if (kf->_features.empty() || (int)kf->_features.size() > ygz_hip_max_keypoints(ctx)) {
        LOG(ERROR) << "StereoMapper::SearchInNeighbors: the keyframe has no features or more than the context holds" << endl;
        return 0;
    }

    auto keypoints = [&](const Frame *f, Keypoints &a) -> bool {
        const size_t n = f->_features.size();
        if (n == 0 || !hip::keypoint_arrays(f, a.px, a.level, a.desc)) return false;
        a.ur.resize(n);
        for (size_t i = 0; i < n; ++i) {
            a.ur[i] = URight(f, i);
            if (!(a.ur[i] >= 0)) a.ur[i] = -1.0;
        }
        return true;
    };
    // a point set from candidates in order, each once; a point Matcher::PointAttributes refuses is skipped
    auto point_set = [&](const std::vector<MapPoint *> &cand, Search &s) {
        std::set<const MapPoint *> seen;
        for (MapPoint *mp : cand)
            if (good(mp) && seen.insert(mp).second) hip::append_point(s, mp);
    };
    ygz_lfuse_params prm;
    ygz_hip_default_lfuse_params(&prm);
    prm.th = _options._fuse_th; prm.baseline = _options._baseline; prm.chi2_mono = _options._fuse_chi2_mono; prm.chi2_stereo = _options._fuse_chi2_stereo;
    const double K4[4] = { (double)cam->fx(), (double)cam->fy(), (double)cam->cx(), (double)cam->cy() };
    // one call: the problems `frames` over the set s; fills s.skip and s.match
    auto search = [&](const std::vector<Frame *> &frames, Search &s, const char *what) -> bool {
        const size_t n = s.points.size(), P = frames.size();
        std::vector<Keypoints> kp(P);
        std::vector<ygz_lfuse_problem> pb(P);
        s.skip.assign(P * n + 1, 0); s.match.assign(P * n + 1, -1);
        for (size_t q = 0; q < P; ++q) {
            if (!keypoints(frames[q], kp[q])) { LOG(ERROR) << "StereoMapper::SearchInNeighbors: a target without usable features" << endl; return false; }
            for (size_t i = 0; i < n; ++i) s.skip[q * n + i] = s.points[i]->_obs.count(frames[q]->_keyframe_id) ? 1 : 0;
            memset(&pb[q], 0, sizeof pb[q]);
            frames[q]->_TCW.to7(pb[q].T);
            pb[q].kp_px = kp[q].px.data(); pb[q].kp_level = kp[q].level.data(); pb[q].kp_desc = kp[q].desc.data(); pb[q].kp_ur = kp[q].ur.data();
            pb[q].pt_skip = &s.skip[q * n]; pb[q].n_kp = (int)kp[q].level.size(); pb[q].set = 0;
        }
        ygz_lfuse_points set;
        set.pw = s.pw.data(); set.pt_desc = s.desc.data(); set.pt_dmax = s.dmax.data(); set.pt_normal = s.normal.data(); set.n_pt = (int)n;
        const bool ok = hip::check(ygz_hip_local_fuse_search(ctx, 1, &set, (int)P, pb.data(), K4, &prm, s.match.data(), nullptr, nullptr, nullptr,
                                                             nullptr, nullptr), what);
        s.skip.resize(P * n); s.match.resize(ok ? P * n : 0);
        return ok;
    };

    // 2. forward: kf's points into every target, one call
    std::vector<MapPoint *> cand;
    for (const Feature *f : kf->_features) if (f) cand.push_back(f->_mappoint);
    point_set(cand, _search[0]);
    _fuse_stats.forward_points = (int)_search[0].points.size();
    std::set<Frame *> touched;
    int fused = 0;
    if (!search(targets, _search[0], "local_fuse_search (forward)")) { _search[0] = Search(); return 0; }
    _targets = targets;
    for (int32_t m : _search[0].match) if (m >= 0) ++_fuse_stats.forward_hits;
    // 3. the walk
    fused += Walk(targets, _search[0], touched);

    // 4. reverse: the targets' points into kf, one call, the same walk
    cand.clear();
    for (const Frame *t : targets)
        for (const Feature *f : t->_features) if (f) cand.push_back(f->_mappoint);
    point_set(cand, _search[1]);
    if (_search[1].points.size() > (size_t)YGZ_LFUSE_MAX_PAIRS) {
        Search &s = _search[1];
        _fuse_stats.reverse_cut = (int)(s.points.size() - YGZ_LFUSE_MAX_PAIRS);
        s.points.resize(YGZ_LFUSE_MAX_PAIRS); s.pw.resize(3 * (size_t)YGZ_LFUSE_MAX_PAIRS); s.normal.resize(3 * (size_t)YGZ_LFUSE_MAX_PAIRS);
        s.dmax.resize(YGZ_LFUSE_MAX_PAIRS); s.desc.resize(32 * (size_t)YGZ_LFUSE_MAX_PAIRS);
    }
    _fuse_stats.reverse_points = (int)_search[1].points.size();
    bool reverse_ok = true;
    if (!_search[1].points.empty()) {
        const std::vector<Frame *> self(1, kf);
        reverse_ok = search(self, _search[1], "local_fuse_search (reverse)");
        if (reverse_ok) {
            for (int32_t m : _search[1].match) if (m >= 0) ++_fuse_stats.reverse_hits;
            fused += Walk(self, _search[1], touched);
        }
    }

    // 5. upkeep: the distinctive descriptors of kf's points; the touched keyframes by id, for the caller's UpdateCovisibility
    std::vector<MapPoint *> own;
    std::set<const MapPoint *> seen;
    for (const Feature *f : kf->_features)
        if (f && good(f->_mappoint) && seen.insert(f->_mappoint).second) own.push_back(f->_mappoint);
    if (!own.empty()) _fuse_stats.descriptors = matcher.ComputeDistinctiveDescriptors(own);
    _touched.assign(touched.begin(), touched.end());
    std::sort(_touched.begin(), _touched.end(), [](const Frame *a, const Frame *b) { return a->_keyframe_id < b->_keyframe_id; });
    return reverse_ok ? fused : 0;
}

int StereoMapper::MapPointCulling(Frame *kf)
{
    if (!kf) { LOG(ERROR) << "StereoMapper::MapPointCulling: no keyframe" << endl; return 0; }
    const unsigned long c = kf->_keyframe_id;
    std::vector<MapPoint *> keep;
    int dead = 0;
    auto set_bad = [](MapPoint *p) {                                    // ORB-SLAM2's MapPoint::SetBadFlag
        for (const auto &ob : p->_obs) if (ob.second) ob.second->_mappoint = nullptr;
        p->_obs.clear();
        p->_bad = true;
    };
    for (MapPoint *p : _recent) {
        if (!p || p->_bad) continue;
        if (p->_cnt_visible > 0 && p->GetFoundRatio() < _options._cull_found_ratio) { set_bad(p); ++dead; }
        else if (c >= p->_first_seen + 2 && Observations(p) <= _options._cull_min_obs) { set_bad(p); ++dead; }
        else if (c >= p->_first_seen + 3) continue;
        else keep.push_back(p);
    }
    _recent.swap(keep);
    return dead;
}

}  // namespace ygz
