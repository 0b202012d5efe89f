// The device tables of k_bow_transform and k_bow_match (bow.hip), the context's vocabulary and the kernels' prototypes, for the translation
// units that launch them: bow.hip from host arrays and slot pairs, srk.hip from tables a kernel wrote.  The kernels take only device pointers.
#pragma once
#include "ygz_internal.h"

struct ygz_hip_ctx::Vocab {
    int k = 0, L = 0, n_nodes = 0, n_words = 0;
    void *blob = nullptr;
    int32_t *child_off, *child, *word_id; uint32_t *desc; double *weight;
    int32_t *kp_word = nullptr, *kp_node = nullptr; double *kp_weight = nullptr;       // [F][cells] per resident keypoint
};

struct VocDev { int L; const int32_t *child_off, *child, *word_id; const uint32_t *desc; const double *weight; };

struct BowPair { const uint32_t *d1, *d2; const int32_t *n1, *n2; const double *p1, *p2; int c1, c2; double E[9]; };

// desc_base + slot/set stride; n per set from n_arr (device) or n_fixed
__global__ void k_bow_transform(VocDev V, const uint32_t *__restrict__ desc, const int32_t *__restrict__ n_arr, int n_fixed, size_t set_stride,
                                int levelsup, int32_t *__restrict__ word, double *__restrict__ weight, int32_t *__restrict__ node);

// MODE 0: SearchByBoW, MODE 1: SearchForTriangulation; grid = (ceil(most features of a frame 1 / 256), pairs).  Only the lanes below a pair's c1
// write match12 (a block past c1 returns at once), and counts[pair] is added to, not set
template <int MODE>
__global__ void k_bow_match(const BowPair *__restrict__ pairs, int th_low, float knn_ratio, double eps_dsqr, double fx, double fy, double cx,
                            double cy, int32_t *__restrict__ match12, size_t match_stride, int32_t *__restrict__ counts);
// defined in bow.hip, which instantiates it for the other translation units
extern template __global__ void k_bow_match<0>(const BowPair *__restrict__ pairs, int th_low, float knn_ratio, double eps_dsqr, double fx, double fy,
                                               double cx, double cy, int32_t *__restrict__ match12, size_t match_stride,
                                               int32_t *__restrict__ counts);
