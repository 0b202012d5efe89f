// The device tables of k_strack_search (strack.hip) and its prototype, for the translation units that launch it: strack.hip from host arrays,
// svo.hip from tables a kernel wrote.  The kernel takes only device pointers through these structs.
#pragma once
#include "ygz_internal.h"

struct StIn { double K4[4]; double bf, r_near, r_wide, cos_near; int32_t w, h, L, pad_; };

struct StSetDev { const double *pw; const uint32_t *pt_desc; const int32_t *pt_level; const double *pt_dmax; const double *pt_normal; int32_t n_pt, pad_; };

struct StProbDev {
    const double *kp_px; const int32_t *kp_level; const uint32_t *kp_desc; const double *kp_ur; const uint8_t *kp_taken; const uint8_t *pt_skip;
    int32_t n_kp, set, pt_off, mode, direction, pad_;
    double th;
    double T[7];
};

#define ST_DEV_LANES     256                // points of one block; grid = (ceil(most points of a set / 256), problems)
#define ST_DEV_IDX_BITS  20                 // key = distance << 20 | keypoint index
#define ST_DEV_NO_KEY    0xFFFFFFFFu        // an empty entry of a point's list

// keys [N][YGZ_STRACK_TOPK], the rest [N] (proj [N][3]); problem q writes entries pt_off .. pt_off + n_pt of its set
__global__ void k_strack_search(const StIn *__restrict__ in_, const StSetDev *__restrict__ sets, const StProbDev *__restrict__ probs,
                                uint32_t *__restrict__ keys, int32_t *__restrict__ n_cand, int32_t *__restrict__ n_gated,
                                int32_t *__restrict__ level, int32_t *__restrict__ reason, double *__restrict__ proj);
