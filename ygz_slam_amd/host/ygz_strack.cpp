// ygz::StereoTracker (include/ygz/Algorithm/StereoTracker.h): nothing in the reference.  ORB-SLAM2's TrackWithMotionModel, UpdateLocalKeyFrames
// (without the spanning tree) and SearchLocalPoints / TrackLocalMap on this data model: both searches run on the device through ONE entry
// point (ygz_hip_stereo_track_search, ygz_slam_amd/csrc/strack.hip), the frame is edited on the host from its result.  The spec is DESIGN.md
// section 26.  Every order goes by index, list position or id, never by address.  Error conventions of the other surfaces: a failed call logs
// and returns 0, only a missing device throws.
#include "ygz/Algorithm/StereoTracker.h"
#include "ygz/Algorithm/PoseOptimizer.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include <algorithm>
#include <cstring>

namespace ygz {

namespace {
using hip::good;
Frame *frame_of(unsigned long id, const Feature *f) { return f && f->_frame ? f->_frame : Memory::GetKeyFrame(id); }

int kept(const Frame *f, bool count_bad)
{
    int n = 0;
    for (const Feature *ft : f->_features)
        if (ft && good(ft->_mappoint) && !ft->_mappoint->_obs.empty() && (count_bad || !ft->_bad)) ++n;
    return n;
}
}

void StereoTracker::SetURight(const Frame *frame, const std::vector<double> &u_right) { if (frame) _u_right[frame->_id] = u_right; }
void StereoTracker::ClearURight(const Frame *frame) { if (frame) _u_right.erase(frame->_id); }
void StereoTracker::Clear() { _u_right.clear(); }

const std::vector<double> *StereoTracker::Columns(const Frame *frame) const
{
    const auto it = _u_right.find(frame->_id);
    return it == _u_right.end() ? nullptr : &it->second;
}

// the one device call: current's keypoints against the set in s (mode 0: level and angle, mode 1: dmax and normal; s.taken, s.th and
// s.direction are the caller's).  Fills the outputs of s
bool StereoTracker::Run(Frame *current, Search &s, int mode, const char *what)
{
    const PinholeCamera *cam = Frame::GetCamera();
    const size_t n = s.points.size(), m = current->_features.size();
    std::vector<double> px, ur(m, -1.0), angle(m);
    std::vector<int32_t> level;
    std::vector<uint8_t> desc;
    if (!hip::keypoint_arrays(current, px, level, desc)) { LOG(ERROR) << "StereoTracker: " << what << ": a feature without a descriptor" << endl; return false; }
    const std::vector<double> *col = Columns(current);
    for (size_t j = 0; j < m; ++j) {
        angle[j] = current->_features[j]->_angle;
        if (col && j < col->size() && (*col)[j] >= 0) ur[j] = (*col)[j];
    }
    ygz_strack_points set;
    memset(&set, 0, sizeof set);
    set.pw = s.pw.data(); set.pt_desc = s.desc.data(); set.n_pt = (int)n;
    if (mode == 0) { set.pt_level = s.level.data(); set.pt_angle = s.angle.data(); }
    else { set.pt_dmax = s.dmax.data(); set.pt_normal = s.normal.data(); }
    ygz_strack_problem pb;
    memset(&pb, 0, sizeof pb);
    current->_TCW.to7(pb.T);
    memcpy(s.T, pb.T, sizeof s.T);
    pb.th = s.th; pb.mode = mode; pb.direction = s.direction; pb.set = 0; pb.n_kp = (int)m;
    pb.kp_px = px.data(); pb.kp_level = level.data(); pb.kp_desc = desc.data(); pb.kp_ur = ur.data(); pb.kp_angle = angle.data();
    pb.kp_taken = s.taken.empty() ? nullptr : s.taken.data();
    ygz_strack_params prm;
    ygz_hip_default_strack_params(&prm);
    prm.baseline = _options._baseline; prm.ratio = _options._ratio; prm.th_dist = _options._th_dist;
    prm.check_orientation = _options._check_orientation ? 1 : 0;
    const double K4[4] = { (double)cam->fx(), (double)cam->fy(), (double)cam->cx(), (double)cam->cy() };
    s.match.assign(n + 1, -1); s.dist.assign(n + 1, -1); s.reason.assign(n + 1, -1); s.outcome.assign(n + 1, -1);
    s.n_cand.assign(n + 1, 0); s.n_gated.assign(n + 1, 0); s.proj.assign(3 * n + 3, 0.0);
    std::vector<int32_t> lvl(n + 1, -1);
    const bool ok = hip::check(ygz_hip_stereo_track_search(hip::Runtime::Get().ctx(), 1, &set, 1, &pb, K4, &prm, s.match.data(), s.dist.data(),
                                                           lvl.data(), s.reason.data(), s.outcome.data(), s.n_cand.data(), s.n_gated.data(),
                                                           s.proj.data(), nullptr, s.counts, nullptr), what);
    s.match.resize(ok ? n : 0); s.dist.resize(ok ? n : 0); s.reason.resize(ok ? n : 0); s.outcome.resize(ok ? n : 0);
    s.n_cand.resize(ok ? n : 0); s.n_gated.resize(ok ? n : 0); s.proj.resize(ok ? 3 * n : 0);
    if (mode == 1) { lvl.resize(ok ? n : 0); s.level.swap(lvl); }     // LOCAL: the predicted level
    return ok;
}

int StereoTracker::TrackWithMotionModel(Frame *current, Frame *last, const SE3 &velocity, PoseOptimizer &opt)
{
    Search &s = _search[0];
    s = Search();
    const int local_kf = _stats.local_keyframes;
    _stats = Stats();
    _stats.local_keyframes = local_kf;
    if (!current || !last || !Frame::GetCamera() || current->_features.empty()) {
        LOG(ERROR) << "StereoTracker::TrackWithMotionModel: no frame, no camera or no features" << endl;
        return 0;
    }
    // 1, 2
    current->_TCW = velocity * last->_TCW;
    for (Feature *f : current->_features) if (f) f->_mappoint = nullptr;
    // 3
    for (const Feature *f : last->_features) {
        if (!f || f->_bad || !good(f->_mappoint)) continue;
        if (!hip::append_point(s, f->_mappoint)) continue;
        s.level.push_back(std::max(f->_level, 0));
        s.angle.push_back(f->_angle);
    }
    _stats.motion_points = (int)s.points.size();
    if (s.points.empty()) return 0;
    // 4
    const std::vector<double> *col = Columns(current);
    bool stereo = false;
    if (col) for (size_t j = 0; j < col->size() && j < current->_features.size(); ++j) stereo = stereo || (*col)[j] >= 0;
    if (stereo) {
        const Vector3d t_lc = last->_TCW.rotation_matrix() * (-1.0 * (current->_TCW.rotation_matrix().transpose() * current->_TCW.translation())) +
                              last->_TCW.translation();
        s.direction = t_lc[2] > _options._baseline ? 1 : (-t_lc[2] > _options._baseline ? -1 : 0);
    }
    _stats.direction = s.direction;
    // 5, 6
    s.th = _options._th_motion;
    if (!Run(current, s, 0, "stereo_track_search (motion)")) return 0;
    if (s.counts[0] < _options._min_matches_motion) {
        _stats.retried = 1;
        s.th = 2 * _options._th_motion;
        if (!Run(current, s, 0, "stereo_track_search (motion, retry)")) return 0;
    }
    _stats.motion_matches = s.counts[0];
    if (s.counts[0] < _options._min_matches_motion) return 0;
    // 7
    std::vector<MapPoint *> matched;
    for (size_t i = 0; i < s.points.size(); ++i) {
        const int j = s.match[i];
        if (j < 0 || j >= (int)current->_features.size()) continue;
        current->_features[j]->_mappoint = s.points[i];
        matched.push_back(s.points[i]);
    }
    // 8: found points are counted in TrackLocalMap only
    std::vector<int> found(matched.size());
    for (size_t k = 0; k < matched.size(); ++k) found[k] = matched[k]->_cnt_found;
    _stats.motion_inliers = opt.Optimize(current, col);
    for (size_t k = matched.size(); k-- > 0;) matched[k]->_cnt_found = found[k];
    // 9
    for (Feature *f : current->_features)
        if (f && f->_bad) f->_mappoint = nullptr;
    _stats.motion_kept = kept(current, true);
    return _stats.motion_kept;
}

int StereoTracker::LocalKeyFrames(Frame *current, std::vector<Frame *> *out)
{
    if (!current || !out) { LOG(ERROR) << "StereoTracker::LocalKeyFrames: no frame or no list" << endl; return 0; }
    out->clear();
    std::map<unsigned long, std::pair<Frame *, int>> votes;             // by keyframe id
    for (const Feature *f : current->_features) {
        if (!f || !good(f->_mappoint)) continue;
        for (const auto &ob : f->_mappoint->_obs) {
            Frame *kf = frame_of(ob.first, ob.second);
            if (!kf) continue;
            auto &v = votes[ob.first];
            v.first = kf; ++v.second;
        }
    }
    Frame *best = nullptr;
    int best_votes = 0;
    for (const auto &v : votes) {                                        // id order: a tie stays with the smaller id
        if (v.second.second > best_votes) { best = v.second.first; best_votes = v.second.second; }
        if (!v.second.first->_bad) out->push_back(v.second.first);
    }
    const size_t voters = out->size();
    for (size_t k = 0; k < voters && (int)out->size() < _options._local_keyframes_max; ++k) {
        const Frame *kf = (*out)[k];
        int looked = 0;
        for (Frame *c : kf->_cov_keyframes) {
            if (looked++ >= _options._neighbours) break;
            if (!c || c->_bad || std::find(out->begin(), out->end(), c) != out->end()) continue;
            out->push_back(c);
            break;
        }
    }
    if (best) current->_ref_keyframe = best;
    _stats.local_keyframes = (int)out->size();
    return (int)out->size();
}

int StereoTracker::TrackLocalMap(Frame *current, const std::vector<Frame *> &local_keyframes, PoseOptimizer &opt)
{
    Search &s = _search[1];
    s = Search();
    _stats.local_on_frame = _stats.local_points = _stats.local_cut = _stats.local_searched = _stats.local_matches = 0;
    _stats.local_inliers = _stats.local_kept = 0;
    if (!current || !Frame::GetCamera() || current->_features.empty()) {
        LOG(ERROR) << "StereoTracker::TrackLocalMap: no frame, no camera or no features" << endl;
        return 0;
    }
    // 1
    std::set<const MapPoint *> seen;
    s.taken.assign(current->_features.size(), 0);
    for (size_t j = 0; j < current->_features.size(); ++j) {
        const Feature *f = current->_features[j];
        if (!f || !good(f->_mappoint)) continue;
        s.taken[j] = 1;
        if (seen.insert(f->_mappoint).second) { ++f->_mappoint->_cnt_visible; ++_stats.local_on_frame; }
    }
    // 2, 3
    for (const Frame *kf : local_keyframes) {
        if (!kf) continue;
        for (const Feature *f : kf->_features) {
            if (!f || !good(f->_mappoint) || !seen.insert(f->_mappoint).second) continue;
            if ((int)s.points.size() >= YGZ_STRACK_MAX_PAIRS) { ++_stats.local_cut; continue; }
            hip::append_point(s, f->_mappoint);
        }
    }
    _stats.local_points = (int)s.points.size();
    // 4, 5
    s.th = _options._th_local;
    const std::vector<double> *col = Columns(current);
    if (!s.points.empty()) {
        if (!Run(current, s, 1, "stereo_track_search (local)")) return 0;
        // 6, 7
        for (size_t i = 0; i < s.points.size(); ++i) {
            MapPoint *mp = s.points[i];
            if (s.reason[i] == 0) { ++mp->_cnt_visible; mp->_track_in_view = true; }
            else mp->_track_in_view = false;
            const int j = s.match[i];
            if (j >= 0 && j < (int)current->_features.size()) current->_features[j]->_mappoint = mp;
        }
        _stats.local_searched = s.counts[1];
        _stats.local_matches = s.counts[0];
    }
    // 8, 9
    _stats.local_inliers = opt.Optimize(current, col);
    _stats.local_kept = kept(current, false);
    return _stats.local_kept;
}

}  // namespace ygz
