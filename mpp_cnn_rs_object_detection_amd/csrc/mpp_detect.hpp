// mpp_detect.hpp -- the CNN-only baseline's detection step (csrc/mpp_detect.hip): threshold + exact greedy distance NMS
// over a whole score map, and the argmax mark classes at a list of pixels.  Host-side driver; the C entries
// (mpp_detect_centers, mpp_mark_classes) are thin wrappers in mpp_api_nets.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#define MPP_DETECT_MAX_NMS 32.0      // largest nms_distance: the halo of a 64 x 64 tile is floor(nms_distance) pixels
#define MPP_DETECT_E_FULL (-13)      // the output buffer is too small; *n_kept has the number needed

// device workspace of the detection pass, kept by the ctx between calls (grown, never shrunk)
struct DetectWs {
  uint8_t *state = nullptr;          // [H*W] per pixel: none / undecided / kept / removed
  size_t state_bytes = 0;
  uint8_t *tile_flag = nullptr;      // [tiles]: the tile still holds undecided candidates
  size_t flag_bytes = 0;
  unsigned long long *counters = nullptr;   // [0] candidates, [1] undecided after a resolve launch, [2] kept
  unsigned long long *keys = nullptr;       // [2][n] sort keys of the kept pixels (radix sort ping-pong)
  size_t key_count = 0;
  unsigned char *sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  int launches = 0;                  // resolve launches of the last mpp_detect_centers
};

int mpp_detect_run(hipStream_t st, DetectWs *ws, int H, int W, int ld, const float *det, double threshold, int strict,
                   double nms_distance, int cap, int32_t *xy, float *scores, int64_t *n_candidates, int64_t *n_kept,
                   std::string *err);
void mpp_detect_free(DetectWs *ws);
void mpp_launch_mark_classes(hipStream_t st, int H, int W, int ld, const float *m0, const float *m1, const float *m2, int n,
                             const int32_t *xy, int32_t *classes);
