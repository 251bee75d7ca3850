// mpp_train.hpp -- training the U-Nets (csrc/mpp_train.hip): the batch builder (crop, augmentation, labels) and the two
// fused losses with their gradients.  Host-side launchers; the C entries (mpp_train_batch, mpp_posnet_loss,
// mpp_shapenet_loss) are thin wrappers in mpp_api_nets.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/mpp_hip.h"

// device workspace of the loss kernels, kept by the ctx between calls (grown, never shrunk)
struct TrainWs {
  double *part = nullptr;            // [workgroups][8] partial sums of one loss launch
  size_t part_count = 0;
  unsigned *done = nullptr;          // workgroups finished; the last one reduces the partials and resets it to 0
  float *lut = nullptr;              // [lut_patches][3][256] histogram-matching tables of one batch (MPP_AUG_HISTMATCH)
  size_t lut_patches = 0;
  float *spat = nullptr;             // [B][2][3][P][P] the patch buffers of k_aug_spatial (MPP_AUG_SPATIAL)
  size_t spat_floats = 0;
  const uint32_t *hist = nullptr;    // [hist_images][3][256] of the resident images, borrowed (mpp_train_set_histograms)
  int hist_images = 0;
};

hipError_t mpp_train_ws_reserve(TrainWs *ws, size_t workgroups);
void mpp_train_ws_free(TrainWs *ws);
hipError_t mpp_launch_train_batch(hipStream_t st, TrainWs *ws, const mpp_train_data &data, const mpp_train_labels &labels,
                                  int B, int P, const int32_t *desc, int flags, uint32_t seed, uint32_t epoch, uint32_t batch,
                                  const mpp_train_out &out);
hipError_t mpp_launch_aug_params(hipStream_t st, int flags, uint32_t seed, uint32_t epoch, uint32_t batch, int B, int P,
                                 int n_images, mpp_aug_record *out);

// error-density resampling and the image histograms (csrc/mpp_resample.hip); the C entries in mpp_api_nets.hip check the arguments
hipError_t mpp_launch_image_histograms(hipStream_t st, const mpp_train_data &data, uint32_t *hist);
hipError_t mpp_launch_error_map(hipStream_t st, int H, int W, int ldh, int ldw, const float *out, int cx0, int cy0, int x0,
                                int x1, int y0, int y1, const int32_t *centers, int n, double max_distance, uint8_t *dens,
                                unsigned long long *sum, float *cell_out);
hipError_t mpp_launch_density_prefix(hipStream_t st, int n_images, const int32_t *img_hw, const int64_t *cell_off,
                                     const int64_t *row_off, int64_t total_rows, const uint8_t *dens, uint32_t *cellcum,
                                     unsigned long long *rowcum);
hipError_t mpp_launch_density_anchors(hipStream_t st, int n_images, const int32_t *img_hw, const int64_t *cell_off,
                                      const int64_t *row_off, const uint32_t *cellcum, const unsigned long long *rowcum, int n,
                                      const int32_t *rows, uint32_t seed, uint32_t epoch, int32_t *anchors);
hipError_t mpp_launch_posnet_loss(hipStream_t st, TrainWs *ws, int B, int P, const float *out, const float *vec,
                                  const float *mask, const float *dil, const double *sums, int with_div, const float *w,
                                  const float *b, float *grad, double *res);
hipError_t mpp_launch_shapenet_loss(hipStream_t st, TrainWs *ws, int B, int P, int n_classes, const float *l0,
                                    const float *l1, const float *l2, const uint8_t *cls, const uint8_t *cover,
                                    const double *sums, float *g0, float *g1, float *g2, double *res);
