// mpp_resample.hip -- what the U-Net trainer resamples its patches from: the per-image colour histograms behind
// MPP_AUG_HISTMATCH, and PosNet's error densities with their integer prefix tables and the anchors drawn from them.
//
//  * k_image_hist: a slice of one image per workgroup, 3 x 256 LDS counters, then integer atomics on the image's table.
//  * k_error_map: one workgroup per tile of 8 x 8 cells (64 x 64 pixels) of a core.  It walks the image's object table in
//    chunks, compacts the centres within max_distance of the tile into LDS and lowers every pixel's nearest squared
//    distance against the list whenever the list fills, so an image may hold any number of objects.  A cell's 64 errors
//    are summed by four lanes in a fixed order; the density sum is an integer atomic.
//  * k_density_rows / k_density_images: inclusive integer prefixes, within each row of cells and over the row totals.
//  * k_density_anchors: one thread per plan row: a 64-bit Philox word, mulhi64 against the image's total, two binary searches.
// Everything summed across workgroups is an integer, so every result repeats bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "mpp_device.hpp"
#include "mpp_train.hpp"
#include "mpp_unet_math.hpp"

namespace {

constexpr int TB = 256;
constexpr int CELL = 8;                    // pixels per cell side (the reference's rescale_fac 1/8)
constexpr int TILE = 8;                    // cells per tile side
constexpr int LCAP = 1024;                 // centres held in LDS between two passes over the pixels
constexpr int HIST_SLICE = 1 << 16;        // pixels of an image per workgroup of k_image_hist

__global__ __launch_bounds__(TB) void k_image_hist(mpp_train_data data, uint32_t *hist) {
  __shared__ uint32_t cnt[3][256];
  const int img = blockIdx.y;
  const size_t npix = (size_t)data.img_hw[2 * img] * (size_t)data.img_hw[2 * img + 1];
  const size_t p0 = (size_t)blockIdx.x * HIST_SLICE;
  if (p0 >= npix) return;
  const size_t p1 = p0 + HIST_SLICE < npix ? p0 + HIST_SLICE : npix;
  for (int ch = 0; ch < 3; ++ch) cnt[ch][threadIdx.x] = 0u;
  __syncthreads();
  const uint8_t *im = data.images + data.img_off[img];
  for (size_t p = p0 + threadIdx.x; p < p1; p += TB) {
    atomicAdd(&cnt[0][im[3 * p]], 1u);
    atomicAdd(&cnt[1][im[3 * p + 1]], 1u);
    atomicAdd(&cnt[2][im[3 * p + 2]], 1u);
  }
  __syncthreads();
  for (int ch = 0; ch < 3; ++ch) {
    const uint32_t c = cnt[ch][threadIdx.x];
    if (c) atomicAdd(&hist[((size_t)img * 3 + ch) * 256 + threadIdx.x], c);
  }
}

// thread t: cell t / 4 of the tile (row-major), rows 2 (t % 4) and 2 (t % 4) + 1 of that cell: 16 pixels
__global__ __launch_bounds__(TB) void k_error_map(int H, int W, int ldh, int ldw, const float *out, int cx0, int cy0, int x0,
                                                  int x1, int y0, int y1, const int32_t *centers, int n, double max_distance,
                                                  uint8_t *dens, unsigned long long *sum, float *cell_out) {
  __shared__ int l_r[LCAP], l_c[LCAP];
  __shared__ int wave_cnt[TB / 64];
  __shared__ unsigned wave_sum[TB / 64];
  const int cw = (W + CELL - 1) / CELL;
  const int cell_in_tile = threadIdx.x >> 2, part = threadIdx.x & 3;
  const int I = x0 / CELL + blockIdx.y * TILE + cell_in_tile / TILE, J = y0 / CELL + blockIdx.x * TILE + cell_in_tile % TILE;
  // the tile's pixels, grown by the reach of a centre
  const int reach = (int)ceil(max_distance) + 1;
  const int tr0 = x0 + blockIdx.y * TILE * CELL - reach, tr1 = min(x1, x0 + (blockIdx.y + 1) * TILE * CELL) + reach;
  const int tc0 = y0 + blockIdx.x * TILE * CELL - reach, tc1 = min(y1, y0 + (blockIdx.x + 1) * TILE * CELL) + reach;
  const int pr = I * CELL + 2 * part, pc = J * CELL;
  int best[16];
  for (int k = 0; k < 16; ++k) best[k] = 0x7fffffff;
  int held = 0;
  for (int base = 0; base < n; base += TB) {
    {
      const int i = base + (int)threadIdx.x;
      int r = 0, c = 0;
      bool keep = false;
      if (i < n) {
        r = centers[2 * i];
        c = centers[2 * i + 1];
        keep = r >= tr0 && r < tr1 && c >= tc0 && c < tc1;
      }
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) wave_cnt[wave] = __popcll(bal);
      __syncthreads();
      int off = held;
      for (int w = 0; w < wave; ++w) off += wave_cnt[w];
      int total = 0;
      for (int w = 0; w < TB / 64; ++w) total += wave_cnt[w];
      if (keep) {
        const int at = off + __popcll(bal & ((1ull << lane) - 1ull));
        l_r[at] = r;
        l_c[at] = c;
      }
      held += total;
      __syncthreads();
    }
    // lower the distances when the next chunk might not fit, and after the last one
    if (held + TB > LCAP || base + TB >= n) {
      for (int k = 0; k < held; ++k) {
        const int dr0 = l_r[k] - pr, dc0 = l_c[k] - pc;
        for (int q = 0; q < 16; ++q) {
          const int dr = dr0 - (q >> 3), dc = dc0 - (q & 7);
          best[q] = min(best[q], dr * dr + dc * dc);
        }
      }
      held = 0;
      __syncthreads();
    }
  }
  // this thread's 16 errors, then the cell's 64 in the order part 0..3
  double acc = 0.0;
  const bool cell_ok = I * CELL < x1 && J * CELL < y1;
  if (cell_ok) {
    for (int q = 0; q < 16; ++q) {
      const int i = pr + (q >> 3), j = pc + (q & 7);
      if (i >= H || j >= W) continue;
      const bool in = best[q] != 0x7fffffff && !(sqrt((double)best[q]) + 1e-8 > max_distance);
      const float s = sigmf(out[(size_t)2 * ldh * ldw + (size_t)(i - cx0) * ldw + (j - cy0)]);
      acc += (double)fabsf((in ? 1.0f : 0.0f) - s);
    }
  }
  const double a1 = __shfl_down(acc, 1), a2 = __shfl_down(acc, 2), a3 = __shfl_down(acc, 3);
  unsigned d = 0u;
  if (part == 0 && cell_ok) {
    const double tot = ((acc + a1) + a2) + a3;
    const int cnt = min(CELL, H - I * CELL) * min(CELL, W - J * CELL);
    const float cell = (float)(tot / (double)cnt);
    const int lvl = (int)floorf(256.0f * cell);
    d = (unsigned)min(255, max(0, lvl));
    dens[(size_t)I * cw + J] = (uint8_t)d;
    if (cell_out) cell_out[(size_t)I * cw + J] = cell;
  }
  for (int s = 32; s > 0; s >>= 1) d += __shfl_down(d, s);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0ull;
    for (int w = 0; w < TB / 64; ++w) t += wave_sum[w];
    if (t) atomicAdd(sum, t);
  }
}

// the image of global row `row` of the concatenated tables: the last i with row_off[i] <= row
__device__ __forceinline__ int image_of_row(const int64_t *row_off, int n_images, int64_t row) {
  int lo = 0, hi = n_images - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row_off[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// one workgroup per row of cells: cellcum = inclusive prefix of the row
__global__ __launch_bounds__(TB) void k_density_rows(int n_images, const int32_t *img_hw, const int64_t *cell_off,
                                                     const int64_t *row_off, const uint8_t *dens, uint32_t *cellcum) {
  __shared__ uint32_t buf[TB];
  const int64_t row = blockIdx.x;
  const int img = image_of_row(row_off, n_images, row);
  const int cw = (img_hw[2 * img + 1] + CELL - 1) / CELL;
  const size_t at = (size_t)cell_off[img] + (size_t)(row - row_off[img]) * cw;
  uint32_t carry = 0u;
  for (int base = 0; base < cw; base += TB) {
    const int j = base + (int)threadIdx.x;
    buf[threadIdx.x] = j < cw ? (uint32_t)dens[at + j] : 0u;
    __syncthreads();
    for (int s = 1; s < TB; s <<= 1) {
      const uint32_t add = (int)threadIdx.x >= s ? buf[threadIdx.x - s] : 0u;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    if (j < cw) cellcum[at + j] = carry + buf[threadIdx.x];
    carry += buf[TB - 1];
    __syncthreads();
  }
}

// one workgroup per image: rowcum = inclusive prefix of the row totals
__global__ __launch_bounds__(TB) void k_density_images(const int32_t *img_hw, const int64_t *cell_off, const int64_t *row_off,
                                                       const uint32_t *cellcum, unsigned long long *rowcum) {
  __shared__ unsigned long long buf[TB];
  const int img = blockIdx.x;
  const int ch = (img_hw[2 * img] + CELL - 1) / CELL, cw = (img_hw[2 * img + 1] + CELL - 1) / CELL;
  const uint32_t *cc = cellcum + cell_off[img];
  unsigned long long *rc = rowcum + row_off[img];
  unsigned long long carry = 0ull;
  for (int base = 0; base < ch; base += TB) {
    const int i = base + (int)threadIdx.x;
    buf[threadIdx.x] = i < ch ? (unsigned long long)cc[(size_t)i * cw + (cw - 1)] : 0ull;
    __syncthreads();
    for (int s = 1; s < TB; s <<= 1) {
      const unsigned long long add = (int)threadIdx.x >= s ? buf[threadIdx.x - s] : 0ull;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < ch) rc[i] = carry + buf[threadIdx.x];
    carry += buf[TB - 1];
    __syncthreads();
  }
}

__global__ __launch_bounds__(TB) void k_density_anchors(int n_images, const int32_t *img_hw, const int64_t *cell_off,
                                                        const int64_t *row_off, const uint32_t *cellcum,
                                                        const unsigned long long *rowcum, int n, const int32_t *rows,
                                                        uint32_t seed, uint32_t epoch, int32_t *anchors) {
  const int t = blockIdx.x * TB + threadIdx.x;
  if (t >= n) return;
  const int img = rows[2 * t];
  if (img < 0 || img >= n_images) {
    anchors[2 * t] = anchors[2 * t + 1] = -1;
    return;
  }
  const int H = img_hw[2 * img], W = img_hw[2 * img + 1];
  const int ch = (H + CELL - 1) / CELL, cw = (W + CELL - 1) / CELL;
  const unsigned long long *rc = rowcum + row_off[img];
  const unsigned long long total = rc[ch - 1];
  if (total == 0ull) {
    anchors[2 * t] = anchors[2 * t + 1] = -1;
    return;
  }
  uint32_t o[4];
  philox4x32_10((uint32_t)rows[2 * t + 1], 0u, 3u, 0u, seed, epoch, o);
  const unsigned long long w = ((unsigned long long)o[1] << 32) | (unsigned long long)o[0];
  const unsigned long long r = __umul64hi(w, total);         // in [0, total)
  // the first row whose inclusive prefix exceeds r, then the first cell of that row
  int lo = 0, hi = ch - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rc[mid] > r) hi = mid; else lo = mid + 1;
  }
  const int I = lo;
  const uint32_t rr = (uint32_t)(r - (I ? rc[I - 1] : 0ull));
  const uint32_t *cc = cellcum + cell_off[img] + (size_t)I * cw;
  lo = 0; hi = cw - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cc[mid] > rr) hi = mid; else lo = mid + 1;
  }
  anchors[2 * t] = min(CELL * I, H);
  anchors[2 * t + 1] = min(CELL * lo, W);
}

}  // namespace

hipError_t mpp_launch_image_histograms(hipStream_t st, const mpp_train_data &data, uint32_t *hist) {
  hipError_t e = hipMemsetAsync(hist, 0, (size_t)data.n_images * 768 * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  // the grid covers the largest image; workgroups past an image's end leave at once
  int32_t *hw = new int32_t[2 * (size_t)data.n_images];
  e = hipMemcpyAsync(hw, data.img_hw, 2 * (size_t)data.n_images * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  size_t most = 1;
  if (e == hipSuccess)
    for (int i = 0; i < data.n_images; ++i) most = std::max(most, (size_t)hw[2 * i] * (size_t)hw[2 * i + 1]);
  delete[] hw;
  if (e != hipSuccess) return e;
  if (most > 0xffffffffull) return hipErrorInvalidValue;     // the counts are uint32
  const size_t slices = (most + HIST_SLICE - 1) / HIST_SLICE;
  if (data.n_images > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_image_hist, dim3((unsigned)slices, data.n_images), dim3(TB), 0, st, data, hist);
  return hipGetLastError();
}

hipError_t mpp_launch_error_map(hipStream_t st, int H, int W, int ldh, int ldw, const float *out, int cx0, int cy0, int x0,
                                int x1, int y0, int y1, const int32_t *centers, int n, double max_distance, uint8_t *dens,
                                unsigned long long *sum, float *cell_out) {
  const int side = TILE * CELL;
  const dim3 grid((y1 - y0 + side - 1) / side, (x1 - x0 + side - 1) / side);
  hipLaunchKernelGGL(k_error_map, grid, dim3(TB), 0, st, H, W, ldh, ldw, out, cx0, cy0, x0, x1, y0, y1, centers, n, max_distance,
                     dens, sum, cell_out);
  return hipGetLastError();
}

hipError_t mpp_launch_density_prefix(hipStream_t st, int n_images, const int32_t *img_hw, const int64_t *cell_off,
                                     const int64_t *row_off, int64_t total_rows, const uint8_t *dens, uint32_t *cellcum,
                                     unsigned long long *rowcum) {
  hipLaunchKernelGGL(k_density_rows, dim3((unsigned)total_rows), dim3(TB), 0, st, n_images, img_hw, cell_off, row_off, dens,
                     cellcum);
  hipLaunchKernelGGL(k_density_images, dim3(n_images), dim3(TB), 0, st, img_hw, cell_off, row_off, cellcum, rowcum);
  return hipGetLastError();
}

hipError_t mpp_launch_density_anchors(hipStream_t st, int n_images, const int32_t *img_hw, const int64_t *cell_off,
                                      const int64_t *row_off, const uint32_t *cellcum, const unsigned long long *rowcum, int n,
                                      const int32_t *rows, uint32_t seed, uint32_t epoch, int32_t *anchors) {
  hipLaunchKernelGGL(k_density_anchors, dim3((n + TB - 1) / TB), dim3(TB), 0, st, n_images, img_hw, cell_off, row_off, cellcum,
                     rowcum, n, rows, seed, epoch, anchors);
  return hipGetLastError();
}
