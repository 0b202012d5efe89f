// How associations become k_pose_opt's edges and how its verdicts get back, for the trackers on resident slots: svo.hip, slm.hip and
// srk.hip; strack.hip's host resolve takes the rotation rule from here.  The including file sets `#pragma clang fp contract(off)` before it
// uses these.  No LDS is declared here and nothing waits on a counter: a kernel that compacts owns its s_wave array and its barriers.
#pragma once
#include "ygz_internal.h"
#include "pose_block.h"

#define YGZ_SLOT_MAX_CELLS 32768         // the taken bitmap of a pair or of a frame: 4 KiB of LDS

// a slot's own keypoint count, clamped to [0, cells]
__device__ __forceinline__ int ygz_slot_count(const int32_t *n_kp, int slot, int cells) { return min(max(n_kp[slot], 0), cells); }

// the edges of problem f: [f * cells, edge_end[f]); edge_of and the two outputs are in the order of what was compacted, [n_problems][cells].
// The order of the fields is part of the three kernels' argument layout: k_slm_resolve measured 1 to 2.6 % slower with edge_of in front
struct SlotEdges {
    double *e_pw, *e_obs; int32_t *e_level; uint8_t *e_kind; const uint8_t *e_outlier; const double *e_chi2;
    int32_t *edge_of, *edge_end;
    uint8_t *out_outlier; double *out_chi2;
};

inline void ygz_slot_edges_bind(SlotEdges &E, uint8_t *dev, const YgzPoseBlock &b, size_t o_out, size_t o_chi2)
{
    E.e_pw = ygz_at<double>(dev, b.e_pw); E.e_obs = ygz_at<double>(dev, b.e_obs); E.e_level = ygz_at<int32_t>(dev, b.e_level);
    E.e_kind = dev + b.e_kind; E.e_outlier = dev + b.e_outlier; E.e_chi2 = ygz_at<const double>(dev, b.e_chi2);
    E.edge_of = ygz_at<int32_t>(dev, b.edge_of); E.edge_end = ygz_at<int32_t>(dev, b.edge_end);
    E.out_outlier = dev + o_out; E.out_chi2 = ygz_at<double>(dev, o_chi2);
}

// the bin of a rotation r in degrees, already rounded to float (step 9 of tests/strack_ref.c; yo_bow_orientation's round(rot / 30) with the
// reference's factor, 30 -> 0), or -1 outside the histogram
__host__ __device__ __forceinline__ int ygz_rot_bin_of(float r)
{
    if (r < 0) r += 360;
    const float fb = r * (1.0f / 30);
    if (!(fb >= 0) || !(fb < 64.0f)) return -1;                          // a bin past 29 has no counter; nothing is converted that an int cannot hold
    int bin = (int)((double)fb + 0.5);                                   // round of a value >= 0: half away from zero
    if (bin == 30) bin = 0;
    return bin < 30 ? bin : -1;
}

// the bin of the rotation between two resident keypoints, whose angles are floats: their difference is formed in double
__host__ __device__ __forceinline__ int ygz_rot_bin(float a1, float a2) { return ygz_rot_bin_of((float)((double)a1 - (double)a2)); }

// the three maxima of the 30-bin histogram, the second and the third dropped below a tenth of the first; for one lane
__host__ __device__ __forceinline__ void ygz_rot_top3(const int *hist, int *ind)
{
    int max1 = 0, max2 = 0, max3 = 0, i0 = -1, i1 = -1, i2 = -1;
    for (int b = 0; b < 30; ++b) {
        const int s = hist[b];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i2 = i1; i1 = i0; i0 = b; }
        else if (s > max2) { max3 = max2; max2 = s; i2 = i1; i1 = b; }
        else if (s > max3) { max3 = s; i2 = b; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i1 = -1; i2 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i2 = -1; }
    ind[0] = i0; ind[1] = i1; ind[2] = i2;
}

// one step of LANES entries of the order-preserving compaction: the place among the problem's edges of the lane's entry if it `has` one.
// Ballot and popcount per wavefront into the caller's s_wave [LANES / 64], one barrier, the wavefronts before this one, and `running`
// moves past the step.  The caller ends its loop body with a second barrier before s_wave is written again
template <int LANES> __device__ __forceinline__ int ygz_edge_slot(bool has, int &running, int *s_wave)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(has);
    if (lane == 0) s_wave[wv] = __popcll(bal);
    __syncthreads();
    int before = running, total = 0;
#pragma unroll
    for (int w = 0; w < LANES / 64; ++w) { const int c = s_wave[w]; if (w < wv) before += c; total += c; }
    running += total;
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

// edge ge: the point X, the observation (px, ur) at `level`; stereo where the keypoint has a right column
__device__ __forceinline__ void ygz_edge_write(const SlotEdges &E, size_t ge, const double *X, const double *px, double ur, int level)
{
    E.e_pw[3 * ge] = X[0]; E.e_pw[3 * ge + 1] = X[1]; E.e_pw[3 * ge + 2] = X[2];
    E.e_obs[3 * ge] = px[0]; E.e_obs[3 * ge + 1] = px[1]; E.e_obs[3 * ge + 2] = ur;
    E.e_level[ge] = level;
    E.e_kind[ge] = ur >= 0 ? 2 : 1;
}

// outlier and chi2 of entry g's edge back to the order of what was compacted (0 and -1.0 without an edge); returns the outlier byte
__device__ __forceinline__ uint8_t ygz_edge_scatter(const SlotEdges &E, size_t base, size_t g, int cells)
{
    const int e = E.edge_of[g];
    const bool has = e >= 0 && e < cells;
    const uint8_t out = has ? E.e_outlier[base + e] : 0;
    E.out_outlier[g] = out;
    E.out_chi2[g] = has ? E.e_chi2[base + e] : -1.0;
    return out;
}
