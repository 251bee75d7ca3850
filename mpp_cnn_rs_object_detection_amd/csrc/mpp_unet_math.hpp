// mpp_unet_math.hpp -- the per-pixel float32 arithmetic of the U-Nets' score maps, stated once for the inference epilogues
// (mpp_maps.hip: planar and channels-last), the training loss (mpp_train.hip) and the error map (mpp_resample.hip).  The planar
// and the channels-last epilogues agree bit for bit, and the loss forms the same float32 values, because they all call these
// functions: every one is inlined, and the build forms no FMA (-ffp-contract=off), so only the addressing differs per caller.
#pragma once
#include "mpp_device.hpp"

// the float32 sigmoid as torch forms it
__device__ __forceinline__ float sigmf(float x) { return 1.0f / (1.0f + expf(-x)); }

// torch.gradient along one axis of n elements at index i: one-sided at both ends, central inside; at(k) = element k
template <class At> __device__ __forceinline__ float grad1(At at, int n, int i) {
  float g;
  if (n == 1) g = 0.f;
  else if (i == 0) g = at(1) - at(0);
  else if (i == n - 1) g = at(i) - at(i - 1);
  else g = (at(i + 1) - at(i - 1)) / 2.0f;
  return g;
}

// PosNet's score at a pixel (pos_net_model.py:186-200, :338-346): the divergence g0 + g1 of the vector field (g0 = d vec0 / d row,
// g1 = d vec1 / d col), x = div * sigmoid(mask logit), q = sigmoid(w x + b), the "div_clf" 1x1 convolution.  Inference keeps q;
// the loss's backward pass needs all four.
struct DivAt { float div, s, x, q; };
__device__ __forceinline__ DivAt div_score(float g0, float g1, float m, float w, float b) {
  DivAt d;
  d.div = g0 + g1;
  d.s = sigmf(m);
  d.x = d.div * d.s;
  d.q = sigmf(w * d.x + b);
  return d;
}
// ... at pixel (x, y) of an H x W output, px(row, col, channel) = element of vec0 / vec1 / mask logit (channel 0 / 1 / 2)
template <class Px> __device__ __forceinline__ DivAt div_at(Px px, int x, int y, int H, int W, float w, float b) {
  const float g0 = grad1([&](int i) { return px(i, y, 0); }, H, x);
  const float g1 = grad1([&](int j) { return px(x, j, 1); }, W, y);
  return div_score(g0, g1, px(x, y, 2), w, b);
}

// softmax over 32 classes held 8 per lane by 4 adjacent lanes (classes 8 q .. 8 q + 7 in lane q of the quad): v <- v's quotients.
// Every lane of the wave calls it (the shuffles).
__device__ __forceinline__ void softmax_quad(float (&v)[8]) {
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < 8; ++i) m = fmaxf(m, v[i]);
  m = fmaxf(m, __shfl_xor(m, 1, WAVE)); m = fmaxf(m, __shfl_xor(m, 2, WAVE));
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) { v[i] = expf(v[i] - m); s += v[i]; }
  s += __shfl_xor(s, 1, WAVE); s += __shfl_xor(s, 2, WAVE);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = v[i] / s;
}

// bfloat16 <-> float32 (round to nearest even, as torch does), and 8 of them in one 16-byte word
__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned int)h << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
  unsigned int u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
__device__ __forceinline__ void unpack_bf16x8(uint4 t, float *v) {
  const unsigned int w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[2 * k] = bf16_to_f32((unsigned short)(w[k] & 0xffffu)); v[2 * k + 1] = bf16_to_f32((unsigned short)(w[k] >> 16)); }
}
__device__ __forceinline__ uint4 pack_bf16x8(const float *v) {
  unsigned int w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = (unsigned int)f32_to_bf16(v[2 * k]) | ((unsigned int)f32_to_bf16(v[2 * k + 1]) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}
