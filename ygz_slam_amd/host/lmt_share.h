// What ygz::LocalMapTracker (ygz_lmt.cpp) and ygz::ResidentMap (ygz_rmap.cpp) share beside lms_gather.h: the attribute and tracking side of
// a list of map points and what a tracked frame leaves on the object graph (step 6).  Both are defined ONCE, in
// ygz_lmt.cpp.  Private to libygz_host.so like surface_share.h.
#ifndef YGZ_HOST_LMT_SHARE_H_
#define YGZ_HOST_LMT_SHARE_H_
#include "ygz/Basic.h"
#include "ygz/Algorithm/LocalMapTracker.h"
#include <unordered_map>
namespace ygz {
namespace hip {

// per point every usable observation in key order (the centre once per distinct frame, in the order the frames are met), the position and
// the descriptor by LocalMapTracker's rule
struct LmtRows {
    std::vector<double> centre, pw;                                // [centres][3], [max(P, 1)][3]
    std::vector<int32_t> off, row_kf, row_level;                   // [P + 1], rows
    std::vector<uint8_t> desc, has_desc;                           // [max(P, 1)][32], [P]
    std::unordered_map<const Frame *, int32_t> centre_at;
    void collect(const std::vector<MapPoint *> &pts);
    // _distinctive_desc when it holds 32 bytes, else the first usable observation's; false: the point has none
    static bool descriptor(const MapPoint *mp, uint8_t out[32]);
};

// the answers of the selection and of the tracking call, frame k's per-point entries at reason + poff[k]
struct LmtTracked {
    const std::vector<MapPoint *> *pts; const std::vector<Frame *> *kfs; bool no_keyframe;
    size_t MP, cells;
    const int32_t *list_pt, *list_len, *prior, *kp_point, *reason; const size_t *poff; const uint8_t *outlier;
    const double *T_out; const int32_t *status, *counts, *inliers, *ref, *n_voters, *n_cut;
    int min_tracked;
};
// step 6 of LocalMapTracker::Track in frame order; the number of tracked frames
int lmt_apply(const std::vector<Frame *> &frames, const LmtTracked &t, std::vector<LocalMapTracker::Result> *results);

}
}
#endif
