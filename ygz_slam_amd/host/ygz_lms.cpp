// ygz::LocalMapSelector (include/ygz/Algorithm/LocalMapSelector.h): nothing in the reference.  StereoTracker::LocalKeyFrames and the point set
// of StereoLocalMap::TrackLocalMap for any number of frames through ONE entry point (ygz_hip_local_map_select, ygz_slam_amd/csrc/lms.hip).  The
// host gathers the object graph into the flat arrays of the call -- the keyframes by _keyframe_id, the points in the order they are met, the
// observations with their feature indices -- and turns the answer back into lists.  The spec is DESIGN.md section 34.  Pointer-keyed tables
// only answer "have I seen this object": every order goes by index, list position or id, never by address.  Error conventions of the other
// surfaces: a failed call logs and returns 0, only a missing device throws.
#include "ygz/Algorithm/LocalMapSelector.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include "lms_gather.h"
#include <algorithm>
#include <map>
#include <unordered_map>

namespace ygz {

namespace hip {
bool lms_select(const char *who, const LmsGather &g, size_t F, int max_keyframes, int max_points, LmsAnswer &a)
{
    ygz_lms_params prm;
    ygz_hip_default_lms_params(&prm);
    prm.max_keyframes = max_keyframes;
    prm.max_points = (int32_t)std::min<int64_t>(max_points, (int64_t)g.P);          // no set is larger than the points of the call
    if (prm.max_points < 1) { LOG(ERROR) << who << ": _max_points below 1" << endl; return false; }
    const size_t K = g.K, E = (size_t)g.fr_off.back();
    a.MP = (size_t)prm.max_points;
    a.ref.assign(F, 0); a.n_voters.assign(F, 0); a.n_local.assign(F, 0); a.local_kf.assign(F * K, 0); a.n_pt.assign(F, 0); a.n_cut.assign(F, 0);
    a.local_pt.assign(F * a.MP, 0); a.prior.assign(std::max<size_t>(E, 1), 0);
    return check(ygz_hip_local_map_select(Runtime::Get().ctx(), (int)K, g.kf_bad.data(), (int)g.C, g.cov.data(), (int)g.P, g.offsets.data(),
                                          g.obs_kf.data(), g.obs_feat.data(), nullptr, (int)F, g.fr_off.data(), g.fr_pt.data(), &prm, nullptr,
                                          a.ref.data(), a.n_voters.data(), a.n_local.data(), a.local_kf.data(), a.n_pt.data(), a.n_cut.data(),
                                          a.local_pt.data(), a.prior.data()), "local_map_select");
}
}

int LocalMapSelector::Select(const std::vector<Frame *> &frames, std::vector<Result> *results)
{
    if (results) results->clear();
    _keyframe_lists.clear();
    _point_lists.clear();
    _stats = Stats();
    if (frames.empty()) { LOG(ERROR) << "LocalMapSelector::Select: no frame" << endl; return 0; }
    for (const Frame *f : frames)
        if (!f) { LOG(ERROR) << "LocalMapSelector::Select: a null frame" << endl; return 0; }
    if (_options._neighbours < 0) { LOG(ERROR) << "LocalMapSelector::Select: _neighbours below 0" << endl; return 0; }
    // 1, 2: the keyframes and the points of the call (lms_gather.h)
    hip::LmsGather g;
    g.gather(frames, _options._neighbours);
    const std::vector<Frame *> &kfs = g.kfs;
    const std::vector<MapPoint *> &pts = g.pts;
    const bool no_keyframe = g.no_keyframe;
    const size_t K = g.K, F = frames.size();
    _stats.dropped = g.dropped;
    _stats.frames = (int)F; _stats.keyframes = (int)kfs.size(); _stats.points = (int)pts.size(); _stats.observations = g.observations;
    // 3
    hip::LmsAnswer ans;
    if (!hip::lms_select("LocalMapSelector::Select", g, F, _options._local_keyframes_max, _options._max_points, ans)) return 0;
    const size_t MP = ans.MP;
    const std::vector<int32_t> &ref = ans.ref, &n_voters = ans.n_voters, &n_local = ans.n_local, &local_kf = ans.local_kf, &n_pt = ans.n_pt,
                               &n_cut = ans.n_cut, &local_pt = ans.local_pt, &prior = ans.prior, &fr_off = g.fr_off;
    // 4: equal lists share one object
    std::map<std::vector<int32_t>, size_t> seen;
    int with_list = 0;
    for (size_t f = 0; f < F; ++f) {
        const int32_t *lk = local_kf.data() + f * K, *lp = local_pt.data() + f * MP;
        const std::vector<int32_t> key(lk, lk + (no_keyframe ? 0 : n_local[f]));
        const auto at = seen.emplace(key, _keyframe_lists.size());
        if (at.second) {
            _keyframe_lists.emplace_back(new std::vector<Frame *>());
            _point_lists.emplace_back(new std::vector<MapPoint *>());
            for (int32_t k : key) _keyframe_lists.back()->push_back(kfs[(size_t)k]);
            for (int i = 0; i < n_pt[f] && !key.empty(); ++i) _point_lists.back()->push_back(pts[(size_t)lp[i]]);
        }
        Frame *best = !no_keyframe && ref[f] >= 0 ? kfs[(size_t)ref[f]] : nullptr;
        if (best) frames[f]->_ref_keyframe = best;
        if (!key.empty()) ++with_list;
        if (!results) continue;
        Result r;
        r.keyframes = _keyframe_lists[at.first->second].get();
        r.points = _point_lists[at.first->second].get();
        r.prior.assign(prior.begin() + fr_off[f], prior.begin() + fr_off[f + 1]);
        r.ref = best; r.voters = n_voters[f]; r.cut = n_cut[f];
        results->push_back(r);
    }
    _stats.lists = (int)_keyframe_lists.size();
    return with_list;
}

}  // namespace ygz
