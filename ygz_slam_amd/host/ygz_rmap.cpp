// ygz::ResidentMap (include/ygz/Algorithm/ResidentMap.h): nothing in the reference.  Upload gathers the object graph with LocalMapTracker's
// own code (lms_gather.h for the selection side, lmt_share.h for the attribute and tracking side) and makes it resident through
// ygz_hip_map_upload; Update pushes a delta through ygz_hip_map_update; Track makes ONE device call, ygz_hip_stereo_local_map_resident, and
// applies its answer with LocalMapTracker's step 6 (lmt_share.h).  The spec is DESIGN.md section 36.  Every order goes by index or list
// position, never by address; the pointer-keyed tables only answer "where is this object in the resident map".  Error conventions of the
// other surfaces: a failed call logs and returns 0, only a missing device throws.
#include "ygz/Algorithm/ResidentMap.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include "lms_gather.h"
#include "lmt_share.h"
#include <algorithm>
#include <cstring>
#include <unordered_map>

namespace ygz {

using hip::good;

struct ResidentMap::Impl {
    ygz_hip_map *map = nullptr;
    bool resident = false;
    std::vector<Frame *> kfs;                                      // the resident keyframes, ascending _keyframe_id
    std::vector<MapPoint *> pts;                                   // the resident points, in the order Upload met them
    std::unordered_map<const MapPoint *, int32_t> pt_at;
    std::unordered_map<const Frame *, int32_t> kf_at, centre_at;
};

ResidentMap::ResidentMap() : _impl(new Impl) {}
ResidentMap::ResidentMap(const Options &options) : _options(options), _impl(new Impl) {}

ResidentMap::~ResidentMap()
{
    if (_impl->map) (void)ygz_hip_map_destroy(hip::Runtime::Get().ctx(), _impl->map);
    delete _impl;
}

bool ResidentMap::Resident() const { return _impl->resident; }

bool ResidentMap::Upload(const std::vector<Frame *> &keyframes)
{
    const char *who = "ResidentMap::Upload";
    if (_options._neighbours < 0) { LOG(ERROR) << who << ": _neighbours below 0" << endl; return false; }
    hip::LmsGather g;
    g.gather_map(keyframes, _options._neighbours);
    if (g.no_keyframe || g.no_point) { LOG(ERROR) << who << ": no keyframe or no point" << endl; return false; }
    hip::LmtRows rows;
    rows.collect(g.pts);
    if (rows.centre.empty()) rows.centre.assign(3, 0.0);                  // no usable observation anywhere: every point gets state 0
    if (rows.row_kf.empty()) { rows.row_kf.push_back(0); rows.row_level.push_back(0); }
    ygz_hip_ctx *c = hip::Runtime::Get().ctx();
    if (!_impl->map && !hip::check(ygz_hip_map_create(c, &_impl->map), "map_create")) return false;
    ygz_map_arrays m;
    memset(&m, 0, sizeof m);
    m.n_keyframes = (int32_t)g.K; m.n_cov = (int32_t)g.C; m.n_points = (int32_t)g.P; m.n_centres = (int32_t)(rows.centre.size() / 3);
    m.kf_bad = g.kf_bad.data(); m.cov = g.cov.data(); m.offsets = g.offsets.data(); m.kf = g.obs_kf.data(); m.feat = g.obs_feat.data();
    m.pt_bad = nullptr;                                                   // a bad point is not gathered
    m.centre = rows.centre.data(); m.a_offsets = rows.off.data(); m.a_kf = rows.row_kf.data(); m.a_level = rows.row_level.data();
    m.pw = rows.pw.data(); m.pt_desc = rows.desc.data(); m.pt_has_desc = rows.has_desc.data();
    std::vector<int32_t> state(g.P, 0);
    if (!hip::check(ygz_hip_map_upload(c, _impl->map, &m, nullptr, nullptr, state.data()), "map_upload")) return false;
    _impl->kfs = g.kfs; _impl->pts = g.pts;
    _impl->pt_at.clear(); _impl->kf_at.clear();
    for (size_t p = 0; p < g.pts.size(); ++p) _impl->pt_at.emplace(g.pts[p], (int32_t)p);
    for (size_t k = 0; k < g.kfs.size(); ++k) _impl->kf_at.emplace(g.kfs[k], (int32_t)k);
    _impl->centre_at = rows.centre_at;
    _impl->resident = true;
    _stats.keyframes = (int)g.kfs.size(); _stats.points = (int)g.pts.size(); _stats.observations = g.observations; _stats.dropped = g.dropped;
    _stats.centres = (int)rows.centre_at.size(); _stats.attribute_rows = (int)rows.off.back();
    _stats.refused = 0;
    for (size_t p = 0; p < g.pts.size(); ++p) _stats.refused += state[p] != 1 || !rows.has_desc[p];
    ++_stats.uploads;
    return true;
}

int ResidentMap::Update(const std::vector<MapPoint *> &points, const std::vector<Frame *> &keyframes)
{
    const char *who = "ResidentMap::Update";
    _stats.skipped = 0;
    if (!_impl->resident) { LOG(ERROR) << who << ": no resident map" << endl; return 0; }
    std::vector<int32_t> pi, ki, ci;
    std::vector<double> pw, centre;
    std::vector<uint8_t> desc, pbad, has, kbad, seen_p(_impl->pts.size(), 0), seen_k(_impl->kfs.size(), 0), seen_c(_impl->centre_at.size(), 0);
    for (const MapPoint *mp : points) {
        const auto at = mp ? _impl->pt_at.find(mp) : _impl->pt_at.end();
        if (at == _impl->pt_at.end()) { ++_stats.skipped; continue; }
        if (seen_p[(size_t)at->second]) continue;                         // named twice: pushed once
        seen_p[(size_t)at->second] = 1;
        pi.push_back(at->second);
        for (int k = 0; k < 3; ++k) pw.push_back(mp->_pos_world[k]);
        desc.resize(desc.size() + 32, 0);
        has.push_back(hip::LmtRows::descriptor(mp, &desc[desc.size() - 32]) ? 1 : 0);
        pbad.push_back(mp->_bad ? 1 : 0);
    }
    for (Frame *kf : keyframes) {
        const auto k = kf ? _impl->kf_at.find(kf) : _impl->kf_at.end();
        const auto cc = kf ? _impl->centre_at.find(kf) : _impl->centre_at.end();
        if (k == _impl->kf_at.end() && cc == _impl->centre_at.end()) { ++_stats.skipped; continue; }
        if (k != _impl->kf_at.end() && !seen_k[(size_t)k->second]) {
            seen_k[(size_t)k->second] = 1;
            ki.push_back(k->second); kbad.push_back(kf->_bad ? 1 : 0);
        }
        if (cc != _impl->centre_at.end() && !seen_c[(size_t)cc->second]) {
            seen_c[(size_t)cc->second] = 1;
            ci.push_back(cc->second);
            const Vector3d v = kf->GetCamCenter();
            for (int i = 0; i < 3; ++i) centre.push_back(v[i]);
        }
    }
    if (pi.empty() && ki.empty() && ci.empty()) return 0;
    ygz_hip_ctx *c = hip::Runtime::Get().ctx();
    if (!hip::check(ygz_hip_map_update(c, _impl->map, (int)pi.size(), pi.data(), pw.data(), desc.data(), pbad.data(), has.data(), (int)ki.size(),
                                       ki.data(), kbad.data(), (int)ci.size(), ci.data(), centre.data()), "map_update"))
        return 0;
    ++_stats.updates;
    return (int)(pi.size() + std::max(ki.size(), ci.size()));
}

int ResidentMap::Track(const std::vector<Frame *> &frames, std::vector<Result> *results)
{
    if (results) results->clear();
    _stats.frames = 0; _stats.unknown = 0; _stats.removed = 0;
    const char *who = "ResidentMap::Track";
    const size_t n = frames.size();
    if (n == 0 || !Frame::GetCamera()) { LOG(ERROR) << who << ": no frame or no camera" << endl; return 0; }
    for (size_t k = 0; k < n; ++k)
        if (!frames[k] || std::find(frames.begin(), frames.begin() + (long)k, frames[k]) != frames.begin() + (long)k) {
            LOG(ERROR) << who << ": a null or repeated frame" << endl;
            return 0;
        }
    if (!_impl->resident) { LOG(ERROR) << who << ": no resident map" << endl; return 0; }
    hip::Runtime &rt = hip::Runtime::Get();
    ygz_hip_ctx *c = rt.ctx();
    const size_t cells = (size_t)rt.cells();
    if (!hip::loadable(who, frames, cells)) return 0;
    // the points on the frames, in feature order
    std::vector<int32_t> fr_off(1, 0), fr_pt;
    for (const Frame *f : frames) {
        for (const Feature *ft : f->_features) {
            int32_t p = -1;
            if (ft && good(ft->_mappoint)) {
                const auto at = _impl->pt_at.find(ft->_mappoint);
                if (at != _impl->pt_at.end()) p = at->second; else ++_stats.unknown;
            }
            fr_pt.push_back(p);
        }
        fr_off.push_back((int32_t)fr_pt.size());
    }
    if (fr_pt.empty()) fr_pt.push_back(-1);
    std::vector<int32_t> slot;
    if (!hip::load_slots(who, frames, cells, slot)) return 0;
    ygz_lms_params q;
    ygz_hip_default_lms_params(&q);
    q.max_keyframes = _options._local_keyframes_max;
    q.max_points = (int32_t)std::min<int64_t>(_options._max_points, (int64_t)_impl->pts.size());
    if (q.max_points < 1) { LOG(ERROR) << who << ": _max_points below 1" << endl; return 0; }
    const size_t MP = (size_t)q.max_points;
    const StereoLocalMap::Options &o = _options._track;
    ygz_slm_params prm;
    ygz_hip_default_slm_params(&prm);
    prm.baseline = o._baseline; prm.th = o._th; prm.ratio = o._ratio; prm.r_near = o._r_near;
    prm.r_wide = o._r_wide; prm.cos_near = o._cos_near; prm.th_dist = o._th_dist; prm.min_edges = o._min_edges;
    std::vector<double> T(7 * n), T_out(7 * n);
    for (size_t k = 0; k < n; ++k) frames[k]->_TCW.to7(&T[7 * k]);
    std::vector<int32_t> ref(n), n_voters(n), n_cut(n), n_pt(n), local_pt(n * MP), n_removed(n), prior(n * cells), status(n), counts(8 * n),
        kp_point(n * cells), inliers(n), reason(n * MP);
    std::vector<uint8_t> outlier(n * cells);
    if (!hip::check(ygz_hip_stereo_local_map_resident(c, _impl->map, (int)n, slot.data(), T.data(), fr_off.data(), fr_pt.data(), &q, &prm, nullptr,
                                                      ref.data(), n_voters.data(), nullptr, nullptr, n_cut.data(), n_pt.data(), local_pt.data(),
                                                      n_removed.data(), prior.data(), T_out.data(), status.data(), counts.data(), kp_point.data(),
                                                      outlier.data(), nullptr, inliers.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                      nullptr, nullptr, nullptr, reason.data(), nullptr, nullptr, nullptr, nullptr),
                    "stereo_local_map_resident"))
        return 0;
    _stats.frames = (int)n;
    std::vector<size_t> poff(n);
    for (size_t k = 0; k < n; ++k) { poff[k] = k * MP; _stats.removed += n_removed[k]; }
    const hip::LmtTracked t = { &_impl->pts, &_impl->kfs, false, MP, cells, local_pt.data(), n_pt.data(), prior.data(), kp_point.data(), reason.data(),
                                poff.data(), outlier.data(), T_out.data(), status.data(), counts.data(), inliers.data(), ref.data(), n_voters.data(),
                                n_cut.data(), o._min_tracked };
    return hip::lmt_apply(frames, t, results);
}

}  // namespace ygz
