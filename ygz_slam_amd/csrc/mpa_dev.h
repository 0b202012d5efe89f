// The device table of k_mpa_attr (mpa.hip) and its launcher, for the translation units that run it on buffers of their own: mpa.hip on its
// packed block, rmap.hip on a resident map.
#pragma once
#include "ygz_internal.h"

struct MpaDev {
    int P;
    const double *center, *pw;
    const int32_t *offsets, *obs_kf, *obs_level;
    double *dmax, *normal;
    int32_t *state;
};

void ygz_mpa_launch(ygz_hip_ctx *ctx, const MpaDev &A);          // one launch, a lane per point, on ctx->stream
