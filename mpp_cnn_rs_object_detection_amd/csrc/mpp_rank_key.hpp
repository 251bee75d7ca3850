// mpp_rank_key.hpp -- the rank key of a detection candidate, shared by the two restatements of naive_detection /
// utils/nms.py:68-110: k_naive_init (mpp_maps.hip, one workgroup per chain tile) and the whole-map detector (mpp_detect.hip).
// key = ordered_bits(value) << 32 | row-major flat index: the larger key is picked first, ties of value go to the larger index.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// float -> uint32 that orders like the value for every finite float (and +-inf); -0 is folded onto +0 so that equal
// values tie on the index alone.  No value that passes a threshold compare maps to 0 (only a NaN pattern does), so a key
// of 0 can stand for "no candidate".
__device__ __forceinline__ uint32_t ordered_bits(float v) {
  const uint32_t b = __float_as_uint(v == 0.f ? 0.f : v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
