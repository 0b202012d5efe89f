// The keyframe-major index of ygz_hip_local_map_select (lms.hip): per keyframe the (feature, point) pairs of its
// observations, sorted by (feature, point).  Built beside the upload from the point-major CSR the call takes, so that the device walks a
// local keyframe's points in feature order without a sort and without an atomic.  Plain C++ without a HIP header: a host program can
// include it (tests/cpp/lms_index_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#define YGZ_LMS_FEAT_END 32768                   // a feature index is in [0, YGZ_LMS_FEAT_END)

// offsets [n_points + 1], kf and feat [offsets[n_points]]: validated by the caller (kf in [0, K), feat in [0, YGZ_LMS_FEAT_END), offsets
// ascending from 0).  koff [K + 1]: keyframe k's pairs are entries koff[k] .. koff[k + 1] - 1 of kpt (the point) and kft (the feature; kft
// may be null).  Two stable counting passes, by feature and then by keyframe: observations are visited in point order, so equal
// (keyframe, feature) pairs stay in point order.  O(n_obs + K + YGZ_LMS_FEAT_END)
inline void ygz_lms_build_index(int n_points, const int32_t *offsets, const int32_t *kf, const int32_t *feat, int K, int32_t *koff, int32_t *kpt,
                                int32_t *kft)
{
    const size_t n_obs = (size_t)offsets[n_points];
    std::vector<int32_t> at((size_t)YGZ_LMS_FEAT_END + 1, 0), order(n_obs), owner(n_obs);
    for (int p = 0; p < n_points; ++p)
        for (int g = offsets[p]; g < offsets[p + 1]; ++g) { owner[(size_t)g] = p; ++at[(size_t)feat[g] + 1]; }
    for (size_t f = 0; f < (size_t)YGZ_LMS_FEAT_END; ++f) at[f + 1] += at[f];
    for (size_t g = 0; g < n_obs; ++g) order[(size_t)at[(size_t)feat[g]]++] = (int32_t)g;       // by (feature, point)
    for (int k = 0; k <= K; ++k) koff[k] = 0;
    for (size_t g = 0; g < n_obs; ++g) ++koff[(size_t)kf[g] + 1];
    for (int k = 0; k < K; ++k) koff[k + 1] += koff[k];
    std::vector<int32_t> fill(koff, koff + K);
    for (size_t i = 0; i < n_obs; ++i) {
        const size_t g = (size_t)order[i];
        const size_t m = (size_t)fill[(size_t)kf[g]]++;
        kpt[m] = owner[g];
        if (kft) kft[m] = feat[g];
    }
}
