// What ygz_hip_stereo_local_map_slots (slm.hip), ygz_hip_stereo_local_map_indexed (slm_index.hip) and ygz_hip_stereo_local_map_resident
// (rmap.hip) share: ONE host body, ygz_slm_run in slm.hip -- the check list, the packed block, the launch sequence and the copy back -- with
// three sources of the point sets.  By value the sets' arrays go up as they are.  By index the map goes up once with the lists, the packed
// per-list arrays lie in the part of the block that stays on the device, and the source's `index` launches k_slm_index to fill them before
// the five launches, which read both alike.  Resident is by index with everything already on the device: the map's
// arrays are device pointers, and the lists, their lengths and the prior are written by the launches of the source's `resident` hook, which
// runs behind the block's upload and in front of `index`.  The host knows no length then, so every list has the stride as its room.
#pragma once
#include "ygz_internal.h"

struct SlmSetTab { uint64_t pw, desc, dmax, normal; int32_t n_pt, pad_; };     // byte offsets of a set's arrays in the packed block

// k_slm_index: the packed block with the table of its sets, the map and the lists [n_lists][stride]
struct SlmIndexDev {
    uint8_t *block; const SlmSetTab *tab;
    const double *pw; const uint4 *desc; const double *dmax, *normal;
    const int32_t *list_pt;
    int stride;
};

// what the resident hook is given (device pointers into the call's block) and what it hands back (device pointers of its own)
struct SlmResidentDev {
    SlmSetTab *tab;                                  // [n_frames]: the hook's launches write n_pt of every entry
    uint8_t *pt_skip;                                // [n_frames][stride]: the hook's launches zero the first n_pt bytes of every row
    int n_frames, stride, cells;
    const int32_t *list_pt;                          // out: [n_frames][stride], list f is frame f's
    const int32_t *prior;                            // out: [n_frames][cells]
};

struct SlmSource {
    int n_sets = 0;                                  // sets, or lists
    const ygz_strack_points *sets = nullptr;         // by value
    int n_points = 0, stride = 0;                    // by index: the map and the lists
    const double *pw = nullptr; const uint8_t *desc = nullptr; const double *dmax = nullptr, *normal = nullptr;
    const int32_t *list_pt = nullptr, *list_len = nullptr;
    void (*index)(ygz_hip_ctx *ctx, const SlmIndexDev &A, int n_lists, int longest) = nullptr;
    // resident: pw, desc, dmax and normal are device pointers, list_pt and list_len stay null, n_sets is the number of frames
    int (*resident)(ygz_hip_ctx *ctx, void *user, SlmResidentDev &R) = nullptr;
    void *user = nullptr;
    bool indexed() const { return index != nullptr; }
    bool is_resident() const { return resident != nullptr; }
    int n_pt(int s) const { return is_resident() ? stride : indexed() ? list_len[s] : sets[s].n_pt; }
};

struct SlmOutputs {
    double *T_out; int32_t *status, *counts, *kp_point; uint8_t *outlier; double *chi2; int32_t *inliers, *rounds_run, *round_status,
    *round_iterations; double *round_cost_initial, *round_cost_final, *round_lambda; int32_t *match, *dist, *level, *reason, *outcome, *n_cand,
    *n_gated; double *proj;
};

int ygz_slm_run(ygz_hip_ctx *ctx, const SlmSource &src, int n_frames, const int32_t *slot, const int32_t *set, const double *T,
                const int32_t *prior, const ygz_slm_params *params, const SlmOutputs &out);
// slm_index.hip: the launch of k_slm_index, the `index` of both indexed sources
void ygz_slm_launch_index(ygz_hip_ctx *ctx, const SlmIndexDev &A, int n_lists, int longest);
