// mpp_birth.hpp -- the candidate of a pixel, shared by the birth-energy map (mpp_birth_map.hip), which evaluates it, and the
// greedy completion (mpp_birth_complete.hip), which appends it: one statement of the rule for both.
#pragma once
#include "mpp_device.hpp"

// argmax class of a pixel's 32 mark probabilities: first maximum, a NaN wins (np.argmax; the rule of k_mark_classes)
__device__ __forceinline__ int birth_argmax(const MPP_GLOBAL float *row) {
  int am = 0;
  float best = row[0];
  if (!isnan(best))
    for (int j = 1; j < MPP_NCLASS; ++j) {
      const float v = row[j];
      if (isnan(v)) { am = j; break; }
      if (v > best) { best = v; am = j; }
    }
  return am;
}

// the marks of the candidate at pixel (x, y) of a tile W wide: the lower bin edge of each mark map's argmax class
__device__ __forceinline__ void birth_candidate_marks(const DevParams *P, const TileRef &t, int x, int y, int W, double *s,
                                                      double *r, double *a) {
  const size_t pix = ((size_t)x * W + y) * MPP_NCLASS;
  *s = P->maps.edges[0][birth_argmax(t.m[0] + pix)];
  *r = P->maps.edges[1][birth_argmax(t.m[1] + pix)];
  *a = P->maps.edges[2][birth_argmax(t.m[2] + pix)];
}
