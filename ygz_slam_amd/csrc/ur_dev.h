// The right column of a resident keypoint from its depth, for the translation units that gather resident slots: svo.hip, slm.hip and srk.hip.
// FP64, uncontracted: the including file sets `#pragma clang fp contract(off)` before it uses these.
#pragma once
#include "ygz_internal.h"

// a keypoint has a depth when its flag is set and the depth is above zero; a NaN depth compares false
__device__ __forceinline__ bool ygz_kp_has_depth(uint8_t has_mp, double z) { return has_mp != 0 && z > 0; }

// u - bf / z with bf = fx baseline formed once by the caller (PoseOptimizer::URightFromDepth); a negative value is a mono keypoint
__device__ __forceinline__ double ygz_kp_right_column(double u, double z, double bf) { return u - bf / z; }
