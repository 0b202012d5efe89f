// The RANSAC sample sets of three indices (pr_sample_sets of tests/pnp_ref.c: a fresh cv::RNG, per iteration three uniform(0, available)
// draws with the swap-remove of Initializer.cpp:33-49) in a form a device lane can evaluate for a point count n that only the device knows.
// The generator's state chain does not depend on n -- only the `% available` does -- so the 3 * max_iter state words are a table the host
// writes once; a lane then forms the set of its iteration from three words and n with the three-draw partial Fisher-Yates held in registers.
// Plain C++ without a HIP header, so a host program can include it (tests/cpp/cvrng_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YGZ_CVRNG_FN __host__ __device__ __forceinline__
#else
#define YGZ_CVRNG_FN inline
#endif

// cv::RNG::next (OpenCV core/operations.hpp), the state in *s; the generator starts from 0xffffffff
YGZ_CVRNG_FN uint32_t ygz_cvrng_next(uint64_t *s)
{
    *s = (uint64_t)(uint32_t)*s * 4164903690u + (uint32_t)(*s >> 32);
    return (uint32_t)*s;
}

// the first `count` outputs of a fresh generator: word 3 * it + j is draw j of iteration it
inline void ygz_cvrng_words(int count, uint32_t *w)
{
    uint64_t st = 0xffffffffu;
    for (int i = 0; i < count; ++i) w[i] = ygz_cvrng_next(&st);
}

// the three distinct indices of [0, n), n >= 3, that the swap-remove yields for the draws w0, w1, w2.  With avail[i] = i at the start:
//   draw 0 takes r0 = w0 % n and puts avail[n - 1] = n - 1 in its place;
//   draw 1 takes r1 = w1 % (n - 1): n - 1 where r1 == r0, else r1; avail[n - 2], which is n - 1 where r0 == n - 2 and n - 2 otherwise, goes to r1;
//   draw 2 takes r2 = w2 % (n - 2): what went to r1 where r2 == r1, else n - 1 where r2 == r0, else r2.
YGZ_CVRNG_FN void ygz_cvrng_set3(uint32_t w0, uint32_t w1, uint32_t w2, int n, int32_t *s)
{
    const int r0 = (int)(w0 % (uint32_t)n), r1 = (int)(w1 % (uint32_t)(n - 1)), r2 = (int)(w2 % (uint32_t)(n - 2));
    const int moved = r0 == n - 2 ? n - 1 : n - 2;
    s[0] = r0;
    s[1] = r1 == r0 ? n - 1 : r1;
    s[2] = r2 == r1 ? moved : (r2 == r0 ? n - 1 : r2);
}
