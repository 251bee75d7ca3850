// mpp_rescale.hpp -- the anti-aliased rescale of dataset translation (csrc/mpp_rescale.hip): a separable resampler driven by
// two host-built tap tables.  Host-side launcher; the C entry (mpp_rescale) is a thin wrapper in mpp_api_nets.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

// workspace of the rescale, kept by the ctx between calls (grown, never shrunk)
struct RescaleWs {
  unsigned char *dev = nullptr;      // the four tables, then the band of the horizontally filtered rows (float64)
  size_t dev_bytes = 0;
  unsigned char *pin = nullptr;      // pinned host copy of the tables: the caller's arrays are free again when the call returns
  size_t pin_bytes = 0;
  hipEvent_t uploaded = nullptr;     // the last upload from `pin` has finished (waited for before `pin` is rewritten)
  int bands = 0;                     // bands of the last call (option rescale_bands)
};

void mpp_rescale_ws_free(RescaleWs *ws);
// 0, or -1 (bad arguments, text in *err) / -2 (HIP error, text in *err).  src, out, out_f64: device; the tables: host.
int mpp_rescale_run(hipStream_t st, RescaleWs *ws, const uint8_t *src, int H, int W, int64_t pitch, const int32_t *row_idx,
                    const double *row_w, int oh, int Tr, const int32_t *col_idx, const double *col_w, int ow, int Tc,
                    uint8_t *out, double *out_f64, int64_t ws_limit, std::string *err);
