// ygz::LocalMapTracker (include/ygz/Algorithm/LocalMapTracker.h): nothing in the reference.  The object graph is gathered ONCE
// (lms_gather.h, shared with LocalMapSelector), then three device calls: the selection (through hip::lms_select), the attributes of the whole
// map (ygz_hip_map_point_attributes) and the tracking on index lists (ygz_hip_stereo_local_map_indexed).  What is applied to frames and
// points afterwards is step 4 of StereoLocalMap::TrackLocalMap and LocalMapSelector's _ref_keyframe.  The spec is DESIGN.md section 35.
// Every order goes by index or list position, never by address.  Error conventions of the other surfaces: a failed call logs and returns 0,
// only a missing device throws.
#include "ygz/Algorithm/LocalMapTracker.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include "lms_gather.h"
#include "lmt_share.h"
#include <algorithm>
#include <cstring>
#include <set>
#include <unordered_map>

namespace ygz {

namespace {
using hip::good;
bool has32(const Mat &d) { return d.data && d.rows * d.cols * (int)d.elemSize() >= 32; }
}

namespace hip {

bool LmtRows::descriptor(const MapPoint *mp, uint8_t out[32])
{
    const Feature *first = nullptr;
    for (const auto &ob : mp->_obs)
        if (ob.second && ob.second->_frame) { first = ob.second; break; }
    const Mat *d = has32(mp->_distinctive_desc) && mp->_distinctive_desc.rows * mp->_distinctive_desc.cols * (int)mp->_distinctive_desc.elemSize() == 32
                       ? &mp->_distinctive_desc : (first && has32(first->_desc) ? &first->_desc : nullptr);
    if (d) memcpy(out, d->data, 32);
    return d != nullptr;
}

// step 3 of LocalMapTracker::Track: every usable observation in key order, the centre once per distinct frame
void LmtRows::collect(const std::vector<MapPoint *> &pts)
{
    const size_t P = pts.size();
    centre.clear(); row_kf.clear(); row_level.clear(); centre_at.clear();
    pw.assign(3 * std::max<size_t>(P, 1), 0.0); off.assign(1, 0); desc.assign(32 * std::max<size_t>(P, 1), 0); has_desc.assign(P, 0);
    for (size_t p = 0; p < P; ++p) {
        const MapPoint *mp = pts[p];
        for (const auto &ob : mp->_obs) {
            const Feature *f = ob.second;
            if (!f || !f->_frame) continue;
            const auto at = centre_at.emplace(f->_frame, (int32_t)centre_at.size());
            if (at.second) {
                const Vector3d cc = f->_frame->GetCamCenter();
                for (int k = 0; k < 3; ++k) centre.push_back(cc[k]);
            }
            row_kf.push_back(at.first->second);
            row_level.push_back(f->_level);
        }
        off.push_back((int32_t)row_kf.size());
        for (int k = 0; k < 3; ++k) pw[3 * p + k] = mp->_pos_world[k];
        has_desc[p] = descriptor(mp, &desc[32 * p]) ? 1 : 0;
    }
}

// step 6 of LocalMapTracker::Track: the frames and the map points, in frame order
int lmt_apply(const std::vector<Frame *> &frames, const LmtTracked &t, std::vector<LocalMapTracker::Result> *results)
{
    const size_t n = frames.size(), MP = t.MP, cells = t.cells;
    const std::vector<MapPoint *> &pts = *t.pts;
    int tracked = 0;
    if (results) results->resize(n);
    for (size_t k = 0; k < n; ++k) {
        Frame *f = frames[k];
        const int32_t *lp = &t.list_pt[k * MP], *pr = &t.prior[k * cells], *kp = &t.kp_point[k * cells];
        const size_t len = (size_t)t.list_len[k];
        std::set<const MapPoint *> on_frame;
        for (size_t j = 0; j < f->_features.size(); ++j)
            if (pr[j] >= 0 && on_frame.insert(pts[(size_t)lp[pr[j]]]).second) ++pts[(size_t)lp[pr[j]]]->_cnt_visible;
        for (size_t i = 0; i < len; ++i) {
            MapPoint *mp = pts[(size_t)lp[i]];
            if (on_frame.count(mp)) continue;                            // skipped through the prior: not touched
            if (t.reason[t.poff[k] + i] == 0) { ++mp->_cnt_visible; mp->_track_in_view = true; }
            else mp->_track_in_view = false;
        }
        for (size_t j = 0; j < f->_features.size(); ++j)
            if (pr[j] < 0 && kp[j] >= 0 && (size_t)kp[j] < len) f->_features[j]->_mappoint = pts[(size_t)lp[kp[j]]];
        f->_TCW = SE3::from7(&t.T_out[7 * k]);
        for (size_t j = 0; j < f->_features.size(); ++j) {
            Feature *ft = f->_features[j];
            if (kp[j] < 0 || !good(ft->_mappoint)) continue;
            if (hip::apply_verdict(f, ft, t.outlier[k * cells + j] != 0)) ft->_mappoint->_cnt_found++;
        }
        Frame *best = !t.no_keyframe && t.ref[k] >= 0 ? (*t.kfs)[(size_t)t.ref[k]] : nullptr;
        if (best) f->_ref_keyframe = best;
        const bool ok = t.status[k] == 0 && t.inliers[k] >= t.min_tracked;
        if (ok) ++tracked;
        if (!results) continue;
        LocalMapTracker::Result &r = (*results)[k];
        r.status = t.status[k]; r.new_matches = t.counts[8 * k + 6]; r.edges = t.counts[8 * k + 7]; r.inliers = t.inliers[k]; r.tracked = ok;
        r.ref = best; r.voters = t.n_voters[k]; r.cut = t.n_cut[k]; r.points = (int)len;
    }
    return tracked;
}

}  // namespace hip

int LocalMapTracker::Track(const std::vector<Frame *> &frames, std::vector<Result> *results)
{
    if (results) results->clear();
    _stats = Stats();
    _sent = Sent();
    const char *who = "LocalMapTracker::Track";
    const size_t n = frames.size();
    if (n == 0 || !Frame::GetCamera()) { LOG(ERROR) << who << ": no frame or no camera" << endl; return 0; }
    for (size_t k = 0; k < n; ++k)
        if (!frames[k] || std::find(frames.begin(), frames.begin() + (long)k, frames[k]) != frames.begin() + (long)k) {
            LOG(ERROR) << who << ": a null or repeated frame" << endl;
            return 0;
        }
    if (_options._neighbours < 0) { LOG(ERROR) << who << ": _neighbours below 0" << endl; return 0; }
    hip::Runtime &rt = hip::Runtime::Get();
    ygz_hip_ctx *c = rt.ctx();
    const size_t cells = (size_t)rt.cells();
    if (!hip::loadable(who, frames, cells)) return 0;
    // 1, 2: the gather and the selection
    hip::LmsGather g;
    g.gather(frames, _options._neighbours);
    _stats.frames = (int)n; _stats.keyframes = (int)g.kfs.size(); _stats.points = (int)g.pts.size(); _stats.observations = g.observations;
    _stats.dropped = g.dropped;
    hip::LmsAnswer ans;
    if (!hip::lms_select(who, g, n, _options._local_keyframes_max, _options._max_points, ans)) return 0;
    const size_t MP = ans.MP, P = g.pts.size();
    // 3: the attributes of the whole map.  Every usable observation in key order, the centre once per distinct frame
    hip::LmtRows rows;
    rows.collect(g.pts);
    std::vector<double> &centre = rows.centre, &pw = rows.pw, dmax(std::max<size_t>(P, 1), 0.0), normal(3 * std::max<size_t>(P, 1), 0.0);
    std::vector<int32_t> &off = rows.off, &row_kf = rows.row_kf, &row_level = rows.row_level, state(std::max<size_t>(P, 1), 0);
    std::vector<uint8_t> &desc = rows.desc, &has_desc = rows.has_desc;
    _stats.centres = (int)rows.centre_at.size(); _stats.attribute_rows = (int)row_kf.size();
    if (P > 0) {
        if (centre.empty()) centre.assign(3, 0.0);                      // no usable observation anywhere: every point gets state 0
        if (row_kf.empty()) { row_kf.push_back(0); row_level.push_back(0); }
        if (!hip::check(ygz_hip_map_point_attributes(c, (int)(centre.size() / 3), centre.data(), (int)P, pw.data(), off.data(), row_kf.data(),
                                                     row_level.data(), dmax.data(), normal.data(), state.data()), "map_point_attributes"))
            return 0;
    }
    _sent.points = g.pts;
    _sent.dmax.assign(dmax.begin(), dmax.begin() + (long)P); _sent.normal.assign(normal.begin(), normal.begin() + (long)(3 * P));
    _sent.state.assign(state.begin(), state.begin() + (long)P); _sent.has_desc.assign(has_desc.begin(), has_desc.end());
    std::vector<uint8_t> refused(P, 0);
    for (size_t p = 0; p < P; ++p) {
        refused[p] = state[p] != 1 || !has_desc[p];
        if (refused[p]) { ++_stats.refused; dmax[p] = 0; for (int k = 0; k < 3; ++k) normal[3 * p + k] = 0; }
    }
    // 4: the refused points leave the lists; where an entry stood before -> where it stands now
    std::vector<int32_t> list_pt(n * MP, -1), list_len(n, 0), moved(MP);
    std::vector<int32_t> prior(n * cells, -1);
    for (size_t k = 0; k < n; ++k) {
        const int32_t *lp = &ans.local_pt[k * MP];
        const int len = g.no_keyframe ? 0 : ans.n_pt[k];
        int32_t m = 0;
        for (int i = 0; i < len; ++i) {
            if (refused[(size_t)lp[i]]) { moved[(size_t)i] = -1; ++_stats.removed; continue; }
            moved[(size_t)i] = m;
            list_pt[k * MP + (size_t)m++] = lp[i];
        }
        list_len[k] = m;
        for (size_t j = 0; j < frames[k]->_features.size(); ++j) {
            const int32_t at = ans.prior[(size_t)g.fr_off[k] + j];
            prior[k * cells + j] = at >= 0 && at < len ? moved[(size_t)at] : -1;
        }
    }
    // 5: the frames into their slots, then one call
    std::vector<int32_t> slot, list_of(n);
    if (!hip::load_slots(who, frames, cells, slot)) return 0;
    size_t pairs = 0;
    std::vector<size_t> poff(n + 1, 0);
    for (size_t k = 0; k < n; ++k) { list_of[k] = (int32_t)k; pairs += (size_t)list_len[k]; poff[k + 1] = pairs; }
    std::vector<double> T(7 * n), T_out(7 * n);
    for (size_t k = 0; k < n; ++k) frames[k]->_TCW.to7(&T[7 * k]);
    std::vector<int32_t> status(n), counts(8 * n), kp_point(n * cells), inliers(n), reason(pairs + 1);
    std::vector<uint8_t> outlier(n * cells);
    const StereoLocalMap::Options &o = _options._track;
    ygz_slm_params prm;
    ygz_hip_default_slm_params(&prm);
    prm.baseline = o._baseline; prm.th = o._th; prm.ratio = o._ratio; prm.r_near = o._r_near;
    prm.r_wide = o._r_wide; prm.cos_near = o._cos_near; prm.th_dist = o._th_dist; prm.min_edges = o._min_edges;
    if (!hip::check(ygz_hip_stereo_local_map_indexed(c, (int)P, pw.data(), desc.data(), dmax.data(), normal.data(), (int)n, (int)MP, list_pt.data(),
                                                     list_len.data(), (int)n, slot.data(), list_of.data(), T.data(), prior.data(), &prm, T_out.data(),
                                                     status.data(), counts.data(), kp_point.data(), outlier.data(), nullptr, inliers.data(), nullptr,
                                                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, reason.data(), nullptr,
                                                     nullptr, nullptr, nullptr), "stereo_local_map_indexed"))
        return 0;
    // 6: the frames and the map points, in frame order
    const hip::LmtTracked t = { &g.pts, &g.kfs, g.no_keyframe, MP, cells, list_pt.data(), list_len.data(), prior.data(), kp_point.data(), reason.data(),
                                poff.data(), outlier.data(), T_out.data(), status.data(), counts.data(), inliers.data(), ans.ref.data(),
                                ans.n_voters.data(), ans.n_cut.data(), o._min_tracked };
    return hip::lmt_apply(frames, t, results);
}

}  // namespace ygz
