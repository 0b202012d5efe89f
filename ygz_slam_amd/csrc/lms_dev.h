// The device table of the local-map selection kernels (lms.hip) and the launcher of its four launches, for the translation units that run
// the selection on buffers of their own: lms.hip on its packed block, rmap.hip on a resident map.
#pragma once
#include "ygz_internal.h"

struct LmsDev {
    int K, C, max_kf, max_pt;
    const uint8_t *kf_bad, *pt_bad;
    const int32_t *cov, *offsets, *obs, *koff, *kpt, *fr_off, *fr_pt;
    int32_t *votes, *ref, *n_voters, *n_local, *local_kf, *n_pt, *n_cut, *local_pt, *fr_prior;
    uint16_t *rank;                              // [F][K]
    int32_t *cnt, *start, *local_ft;             // [F][K], [F][K + 1], [F][max_pt]
};

// k_lms_vote, k_lms_points, k_lms_place and, with max_len > 0 (the longest frame's entries), k_lms_prior, on ctx->stream
void ygz_lms_launch(ygz_hip_ctx *ctx, const LmsDev &A, int n_frames, int max_len);
