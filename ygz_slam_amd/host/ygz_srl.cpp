// ygz::StereoRelocalizer (include/ygz/Algorithm/StereoRelocalizer.h): nothing in the reference.  ORB-SLAM2's Tracking::Relocalization up to its
// first PoseOptimization for any number of lost frames: the point sets of the candidate keyframes are built on the host, the frames' and
// keyframes' feature lists and depths are put into their slots (hip::load_slots, surface_share.h), then ONE entry point
// (ygz_hip_stereo_relocalize_slots, ygz_slam_amd/csrc/srl.hip) computes the BoW of every slot, searches, claims, removes by orientation, runs the
// P3P RANSAC, optimises and picks the winner on the device, and the frames with a winner are edited from its result in frame order.  The spec
// is DESIGN.md section 32.  Every order goes by index or list position, never by address.  Error conventions of the other surfaces: a failed
// call logs and returns 0, only a missing device throws.
#include "ygz/Algorithm/StereoRelocalizer.h"
#include "ygz/hip/Runtime.h"
#include "ygz_hip.h"
#include "surface_share.h"
#include "retrieval.h"
#include <algorithm>
#include <map>

namespace ygz {

namespace {
using hip::good;

struct PointSet {
    std::vector<MapPoint *> points;
    std::vector<double> pw;
};
}

std::vector<Frame *> StereoRelocalizer::Candidates(Frame *frame, const std::vector<Frame *> &keyframes)
{
    std::vector<Frame *> out;
    if (!frame || Frame::_vocab == nullptr) return out;
    if (frame->_bow_vec.empty()) frame->ComputeBoW();
    if (frame->_bow_vec.empty()) return out;
    std::vector<hip::Retrieved> found;
    hip::bow_candidates(frame, keyframes, _kfdb, _options._max_candidates, _options._min_score_ratio, found);
    for (const hip::Retrieved &r : found) out.push_back(r.kf);
    return out;
}

int StereoRelocalizer::Relocalize(const std::vector<Frame *> &frames, const std::vector<std::vector<Frame *>> &candidates,
                                  std::vector<Result> *results)
{
    static const char *who = "StereoRelocalizer::Relocalize";
    if (results) results->clear();
    const size_t n = frames.size();
    if (n == 0 || candidates.size() != n || !Frame::GetCamera()) {
        LOG(ERROR) << who << ": no frame, no camera, or candidate lists of another length" << endl;
        return 0;
    }
    hip::Runtime &rt = hip::Runtime::Get();
    ygz_hip_ctx *c = rt.ctx();
    const size_t cells = (size_t)rt.cells();
    // 1: the distinct keyframes in the order they first appear, one set each; the ragged candidate lists as offsets and indices
    std::vector<Frame *> kfs;
    std::vector<int32_t> cand_off(1, 0), cand_kf;
    for (size_t k = 0; k < n; ++k) {
        if (!frames[k] || std::find(frames.begin(), frames.begin() + (long)k, frames[k]) != frames.begin() + (long)k) {
            LOG(ERROR) << who << ": a null or repeated frame" << endl;
            return 0;
        }
        for (Frame *kf : candidates[k]) {
            if (!kf || kf == frames[k]) {
                LOG(ERROR) << who << ": a null keyframe, or a frame among its own candidates" << endl;
                return 0;
            }
            const auto it = std::find(kfs.begin(), kfs.end(), kf);
            cand_kf.push_back((int32_t)(it - kfs.begin()));
            if (it == kfs.end()) kfs.push_back(kf);
        }
        cand_off.push_back((int32_t)cand_kf.size());
    }
    const size_t P = cand_kf.size();
    if (P == 0 || kfs.size() > (size_t)YGZ_SRL_MAX_KEYFRAMES || n > (size_t)YGZ_SRL_MAX_FRAMES || P > (size_t)YGZ_SRL_MAX_PROBLEMS) {
        LOG(ERROR) << who << ": no candidate at all, or more frames, keyframes or candidates than the call takes" << endl;
        return 0;
    }
    std::vector<Frame *> all(kfs);                                       // every frame that needs a slot, keyframes first, each once
    for (Frame *f : frames)
        if (std::find(all.begin(), all.end(), f) == all.end()) all.push_back(f);
    if (!hip::loadable(who, all, cells)) return 0;                       // before kf_point is indexed by feature
    std::vector<PointSet> sets(kfs.size());
    std::vector<ygz_strack_points> views(kfs.size());
    std::vector<int32_t> kf_point(kfs.size() * cells, -1), kf_set(kfs.size());
    for (size_t s = 0; s < kfs.size(); ++s) {
        std::map<const MapPoint *, int32_t> index;
        for (size_t i = 0; i < kfs[s]->_features.size(); ++i) {
            const Feature *ft = kfs[s]->_features[i];
            if (!good(ft->_mappoint)) continue;
            const auto at = index.find(ft->_mappoint);
            if (at != index.end()) { kf_point[s * cells + i] = at->second; continue; }
            index[ft->_mappoint] = kf_point[s * cells + i] = (int32_t)sets[s].points.size();
            sets[s].points.push_back(ft->_mappoint);
            for (int k = 0; k < 3; ++k) sets[s].pw.push_back(ft->_mappoint->_pos_world[k]);
        }
        ygz_strack_points &v = views[s];
        v.pw = sets[s].pw.data(); v.pt_desc = nullptr; v.pt_level = nullptr; v.pt_angle = nullptr; v.pt_dmax = nullptr; v.pt_normal = nullptr;
        v.n_pt = (int)sets[s].points.size();
        kf_set[s] = (int32_t)s;
    }
    // 2: the frames into their slots, with their feature lists and depths
    std::vector<int32_t> all_slot;
    if (!hip::load_slots(who, all, cells, all_slot)) return 0;
    // 3: one call
    const std::vector<int32_t> kf_slot(all_slot.begin(), all_slot.begin() + (long)kfs.size());       // `all` begins with the keyframes
    std::vector<int32_t> slot(n), best(n), status(P), counts(10 * P), prior(P * cells);
    std::vector<uint8_t> outlier(P * cells);
    std::vector<double> T_out(7 * n);
    for (size_t k = 0; k < n; ++k) slot[k] = all_slot[(size_t)(std::find(all.begin(), all.end(), frames[k]) - all.begin())];
    ygz_srl_params prm;
    ygz_hip_default_srl_params(&prm);
    prm.baseline = _options._baseline; prm.th_low = _options._th_low; prm.knn_ratio = _options._knn_ratio; prm.levelsup = _options._levelsup;
    prm.check_orientation = _options._check_orientation ? 1 : 0; prm.min_matches = _options._min_matches;
    prm.pnp.max_iter = _options._ransac_iterations; prm.pnp.chi2 = _options._ransac_chi2; prm.pnp.min_inliers = _options._min_ransac_inliers;
    prm.min_final_inliers = _options._min_final_inliers;
    if (!hip::check(ygz_hip_stereo_relocalize_slots(c, (int)views.size(), views.data(), (int)kfs.size(), kf_slot.data(), kf_set.data(),
                                                    kf_point.data(), (int)n, slot.data(), cand_off.data(), cand_kf.data(), &prm, T_out.data(),
                                                    best.data(), status.data(), nullptr, nullptr, nullptr, counts.data(), nullptr, nullptr,
                                                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, prior.data(),
                                                    outlier.data(), nullptr, nullptr, nullptr, nullptr), "stereo_relocalize_slots"))
        return 0;
    // 4: the frames with a winner, in frame order
    int relocalised = 0;
    if (results) results->resize(n);
    for (size_t k = 0; k < n; ++k) {
        Frame *f = frames[k];
        const int32_t q0 = cand_off[k], q1 = cand_off[k + 1], q = best[k];
        if (q >= q0 && q < q1) {
            const PointSet &s = sets[(size_t)cand_kf[(size_t)q]];
            const int32_t *pr = &prior[(size_t)q * cells];
            for (Feature *ft : f->_features) ft->_mappoint = nullptr;
            f->_TCW = SE3::from7(&T_out[7 * k]);
            for (size_t j = 0; j < f->_features.size(); ++j) {
                Feature *ft = f->_features[j];
                if (outlier[(size_t)q * cells + j]) { ft->_bad = true; continue; }
                if (pr[j] < 0 || (size_t)pr[j] >= s.points.size()) continue;
                ft->_mappoint = s.points[(size_t)pr[j]];
                hip::apply_verdict(f, ft, false);
            }
            f->_ref_keyframe = kfs[(size_t)cand_kf[(size_t)q]];
            ++relocalised;
        }
        if (!results) continue;
        Result &r = (*results)[k];
        r.winner = q >= q0 && q < q1 ? (int)(q - q0) : -1;
        for (int32_t p = q0; p < q1; ++p) {
            r.status.push_back(status[(size_t)p]); r.matches.push_back(counts[10 * (size_t)p + 7]);
            r.pnp_inliers.push_back(counts[10 * (size_t)p + 8]); r.final_inliers.push_back(counts[10 * (size_t)p + 9]);
        }
    }
    return relocalised;
}

}  // namespace ygz
