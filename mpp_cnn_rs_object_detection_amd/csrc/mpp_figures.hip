// mpp_figures.hip -- the result pictures of `infer` (NNNN_detection.png, NNNN_gt.png; the reference draws them with OpenCV in
// models/shape_net/display.py:37-59) composed on the device, where the picture and the score maps already are: only the
// finished RGB8 image crosses PCIe.  DESIGN.md section 11 states the rules; in short
//
//   k_outline_scatter  one thread per (rectangle, edge): the integer 8-connected Bresenham walk from corner k to corner
//                      (k + 1) % 4, corners (row, col) int32.  Every pixel of the walk that lies inside the image takes
//                      atomicMax(owner, rectangle index + 1): a pixel crossed by several outlines belongs to the highest
//                      index, which is what drawing the rectangles one after another in list order leaves, whatever order
//                      the threads arrive in.  Pixels outside are skipped one by one -- the line is never clipped, clipping
//                      would move its pixels.  (An edge whose bounding box misses the image plots nothing and returns at once.)
//   k_compose          one thread per pixel: the base colour (the picture's float RGB, or a scalar map clipped to
//                      [vmin, vmax] and looked up in a 256-entry table), replaced by the owner's colour where there is one,
//                      to 8 bits as matplotlib's imsave does it: uint8(v * 255) in float32, truncated; a pixel with a NaN
//                      channel is black.
//
// HBM-bound and tiny next to the chains: 4 B (owner) + 12 B (picture) read and 3 B written per pixel.
#include "mpp_device.hpp"
#include "mpp_launch.hpp"

__global__ __launch_bounds__(256) void k_outline_scatter(const int32_t *corners, int n, int H, int W, int32_t *owner) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 4 * n) return;
  const int r = t >> 2, k = t & 3;
  const int32_t *q = corners + (size_t)r * 8;
  int y0 = q[2 * k], x0 = q[2 * k + 1];
  const int y1 = q[2 * ((k + 1) & 3)], x1 = q[2 * ((k + 1) & 3) + 1];
  // the walk stays inside the bounding box of its end points: nothing to plot when that misses the image
  if (max(y0, y1) < 0 || min(y0, y1) >= H || max(x0, x1) < 0 || min(x0, x1) >= W) return;
  const int dx = abs(x1 - x0), dy = -abs(y1 - y0);           // |coordinate| <= MPP_FIG_COORD_MAX: no overflow below
  const int sx = x0 < x1 ? 1 : -1, sy = y0 < y1 ? 1 : -1;
  int err = dx + dy;
  for (;;) {
    if ((unsigned)y0 < (unsigned)H && (unsigned)x0 < (unsigned)W) atomicMax(&owner[(size_t)y0 * W + x0], r + 1);
    if (x0 == x1 && y0 == y1) break;
    const int e2 = 2 * err;
    if (e2 >= dy) { err += dy; x0 += sx; }
    if (e2 <= dx) { err += dx; y0 += sy; }
  }
}

// v * 255 in float32, truncated (matplotlib's `(xx * 255).astype(np.uint8)` for a float32 picture in 0..1; values outside
// that range, which imsave refuses, are clamped)
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f); }

__global__ __launch_bounds__(256) void k_compose(size_t n_px, const float *rgb, const float *scalar, double vmin, double vmax,
                                                 const float *lut, const int32_t *owner, const float *colors, uint8_t *out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_px) return;
  const int own = owner ? owner[i] : 0;
  const float *src;
  if (own > 0) {
    src = colors + (size_t)(own - 1) * 3;
  } else if (rgb) {
    src = rgb + i * 3;
  } else {
    double v = (double)scalar[i];
    if (!(v >= vmin)) v = vmin;                              // (NaN too)
    if (v > vmax) v = vmax;
    const int idx = (int)((v - vmin) / (vmax - vmin) * 256.0);
    src = lut + 3 * (idx > 255 ? 255 : idx);
  }
  const float a = src[0], b = src[1], c = src[2];
  const bool nan = a != a || b != b || c != c;
  out[i * 3 + 0] = nan ? 0 : to_u8(a);
  out[i * 3 + 1] = nan ? 0 : to_u8(b);
  out[i * 3 + 2] = nan ? 0 : to_u8(c);
}

// All pointers device.  owner: [H][W] int32 workspace, needed (and zeroed here) only when n > 0.
extern "C" hipError_t mpp_launch_draw_outlines(hipStream_t st, int H, int W, const float *rgb, const float *scalar, double vmin,
                                               double vmax, const float *lut, int n, const int32_t *corners, const float *colors,
                                               int32_t *owner, uint8_t *out) {
  const size_t n_px = (size_t)H * W;
  if (n > 0) {
    hipError_t e = hipMemsetAsync(owner, 0, n_px * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_outline_scatter, dim3((4u * (unsigned)n + 255u) / 256u), dim3(256), 0, st, corners, n, H, W, owner);
  }
  hipLaunchKernelGGL(k_compose, dim3((unsigned)((n_px + 255) / 256)), dim3(256), 0, st, n_px, rgb, scalar, vmin, vmax, lut,
                     n > 0 ? owner : (const int32_t *)nullptr, colors, out);
  return hipGetLastError();
}
