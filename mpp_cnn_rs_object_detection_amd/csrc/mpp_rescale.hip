// mpp_rescale.hip -- the anti-aliased rescale of dataset translation (reference data/translation/translate_DOTA.py:181,
// skimage.transform.rescale(anti_aliasing=True) + plt.imsave) as a generic separable resampler:
//
//   out[i][j][c] = sum_t wr[i][t] * ( sum_s wc[j][s] * src[ir[i][t]][ic[j][s]][c] / 255 ),   t and s ascending, float64
//   u8[i][j][c]  = (uint8)(255 * min(max(out, 0), 1))                                        (truncation)
//
// The host folds the Gaussian blur (mirror boundary) and the bilinear interpolation of each axis into one table of
// (source index, weight) pairs per output row / column (dataset_translation.rescale_tables), so the kernels hold no index
// logic and no boundary rule.  Two kernels per band of output rows:
//
//  k_rescale_rows  the horizontal pass, first because it shrinks the data by the scale before anything is written.  A
//                  workgroup of four waves takes 64 output columns (one per lane) of 16 source rows: the columns' taps go to
//                  LDS transposed ([tap][lane]: consecutive lanes read consecutive words), the span of source bytes they
//                  touch is staged in LDS with aligned 16-byte loads along each row, and a thread accumulates its column for
//                  four rows at once, so a weight and an index are read once per four rows.  Writes float64 [row][col][3].
//  k_rescale_cols  the vertical pass.  A workgroup works on one output row, so its taps are the same in every lane and come
//                  through scalar loads; a thread sums two adjacent float64 values (one 16-byte load per tap, contiguous
//                  across the wave), clips, truncates and writes the 8-bit pixel and, on request, the float64 value.
//
// The intermediate holds only the source rows a band's taps name, so the workspace stays under the caller's limit for any
// image; the sum of an output value has one order whatever the band, so the result does not depend on the band height.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpp_rescale.hpp"

namespace {

constexpr int RS_COLS = 64;            // output columns of a workgroup of k_rescale_rows, one per lane
constexpr int RS_WAVES = 4;
constexpr int RS_RPT = 4;              // source rows per thread
constexpr int RS_ROWS = RS_WAVES * RS_RPT;
constexpr int RS_THREADS = RS_COLS * RS_WAVES;
constexpr size_t RS_LDS_MAX = 64 * 1024;

__device__ __forceinline__ uint4 load_chunk(const uint8_t *p, const uint8_t *lo, const uint8_t *hi) {
  if (p >= lo && p + 16 <= hi) return *reinterpret_cast<const uint4 *>(p);
  unsigned v[4] = {0u, 0u, 0u, 0u};    // a chunk that straddles an end of the image: byte by byte, nothing outside is read
  for (int b = 0; b < 16; ++b)
    if (p + b >= lo && p + b < hi) v[b >> 2] |= (unsigned)p[b] << (8 * (b & 3));
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// tmp[r - r0][j][c] = sum_s wc[j][s] * src[r][ic[j][s]][c] / 255 for the source rows r0 <= r < r1.
// Dynamic LDS: double w[T][64] | int idx[T][64] | int minmax[4] | uint8 rows[RS_ROWS][row_stride]
__global__ __launch_bounds__(RS_THREADS) void k_rescale_rows(const uint8_t *__restrict__ src, const uint8_t *src_end, long long pitch,
                                                             int r0, int r1, const int32_t *__restrict__ col_idx,
                                                             const double *__restrict__ col_w, int ow, int T, int row_stride,
                                                             double *__restrict__ tmp, int tpitch) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double *w_l = reinterpret_cast<double *>(lds);
  int *i_l = reinterpret_cast<int *>(lds + (size_t)T * RS_COLS * 8);
  int *mm = i_l + T * RS_COLS;
  unsigned char *rows = reinterpret_cast<unsigned char *>(mm + 4);
  const int tid = threadIdx.x, j0 = blockIdx.x * RS_COLS, rb0 = r0 + blockIdx.y * RS_ROWS;

  if (tid == 0) { mm[0] = INT_MAX; mm[1] = -1; }
  __syncthreads();
  int lo = INT_MAX, hi = -1;
  for (int e = tid; e < T * RS_COLS; e += RS_THREADS) {
    const int jj = e / T, t = e - jj * T;
    const size_t g = (size_t)min(j0 + jj, ow - 1) * T + t;      // columns past the image repeat the last one (never stored)
    const int ix = col_idx[g];
    w_l[t * RS_COLS + jj] = col_w[g];
    i_l[t * RS_COLS + jj] = ix;
    lo = min(lo, ix); hi = max(hi, ix);
  }
  atomicMin(&mm[0], lo);
  atomicMax(&mm[1], hi);
  __syncthreads();
  const int cmin = mm[0];

  // the bytes [cmin * 3, (cmax + 1) * 3) of each row, from the 16-byte boundary below them
  const int nch = row_stride >> 4;
  for (int e = tid; e < RS_ROWS * nch; e += RS_THREADS) {
    const int rb = e / nch, k = e - rb * nch;
    if (rb0 + rb >= r1) continue;
    const uint8_t *a = src + (size_t)(rb0 + rb) * (size_t)pitch + (size_t)cmin * 3;
    const uint8_t *p = a - (reinterpret_cast<uintptr_t>(a) & 15) + (size_t)k * 16;
    *reinterpret_cast<uint4 *>(rows + (size_t)rb * row_stride + (size_t)k * 16) = load_chunk(p, src, src_end);
  }
  __syncthreads();

  const int tx = tid & (RS_COLS - 1), ty = tid / RS_COLS;
  const unsigned char *rp[RS_RPT];
  for (int q = 0; q < RS_RPT; ++q) {
    const int rb = ty * RS_RPT + q;
    const uint8_t *a = src + (size_t)(rb0 + rb) * (size_t)pitch + (size_t)cmin * 3;     // (an address, not dereferenced)
    rp[q] = rows + (size_t)rb * row_stride + (reinterpret_cast<uintptr_t>(a) & 15);
  }
  double acc[RS_RPT][3] = {};
  for (int t = 0; t < T; ++t) {
    const double w = w_l[t * RS_COLS + tx];
    const int o = (i_l[t * RS_COLS + tx] - cmin) * 3;
#pragma unroll
    for (int q = 0; q < RS_RPT; ++q) {
      acc[q][0] = fma(w, (double)rp[q][o], acc[q][0]);
      acc[q][1] = fma(w, (double)rp[q][o + 1], acc[q][1]);
      acc[q][2] = fma(w, (double)rp[q][o + 2], acc[q][2]);
    }
  }
  const int j = j0 + tx;
  if (j >= ow) return;
#pragma unroll
  for (int q = 0; q < RS_RPT; ++q) {
    const int r = rb0 + ty * RS_RPT + q;
    if (r >= r1) break;
    double *d = tmp + (size_t)(r - r0) * tpitch + (size_t)j * 3;
    d[0] = acc[q][0] / 255.0; d[1] = acc[q][1] / 255.0; d[2] = acc[q][2] / 255.0;
  }
}

// out[i][x] = sum_t wr[i][t] * tmp[ir[i][t] - r0][x] for the output rows i0 + blockIdx.y, x = 3 * column + channel
__global__ __launch_bounds__(256) void k_rescale_cols(const double *__restrict__ tmp, int tpitch, int r0,
                                                      const int32_t *__restrict__ row_idx, const double *__restrict__ row_w, int T,
                                                      int i0, int ow3, uint8_t *__restrict__ out, double *__restrict__ out_f64) {
  const int i = i0 + blockIdx.y;
  const int x = 2 * (blockIdx.x * 256 + threadIdx.x);
  if (x >= ow3) return;
  const int32_t *ir = row_idx + (size_t)i * T;
  const double *wr = row_w + (size_t)i * T;
  double a0 = 0.0, a1 = 0.0;
  for (int t = 0; t < T; ++t) {
    // rows of tmp start on 16 bytes (tpitch is even); with ow3 odd the last pair's second value is padding, never stored
    const double2 v = *reinterpret_cast<const double2 *>(tmp + (size_t)(ir[t] - r0) * tpitch + x);
    const double w = wr[t];
    a0 = fma(w, v.x, a0);
    a1 = fma(w, v.y, a1);
  }
  const size_t o = (size_t)i * ow3 + x;
  out[o] = (uint8_t)(255.0 * fmin(fmax(a0, 0.0), 1.0));
  if (out_f64) out_f64[o] = a0;
  if (x + 1 < ow3) {
    out[o + 1] = (uint8_t)(255.0 * fmin(fmax(a1, 0.0), 1.0));
    if (out_f64) out_f64[o + 1] = a1;
  }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

int bad(std::string *err, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  *err = buf;
  return code;
}
#define RS_HIP(call)                                                                                              \
  do {                                                                                                            \
    hipError_t e_ = (call);                                                                                       \
    if (e_ != hipSuccess) return bad(err, -2, "rescale: %s failed: %s", #call, hipGetErrorString(e_));           \
  } while (0)

}  // namespace

void mpp_rescale_ws_free(RescaleWs *ws) {
  if (ws->dev) (void)hipFree(ws->dev);
  if (ws->pin) (void)hipHostFree(ws->pin);
  if (ws->uploaded) (void)hipEventDestroy(ws->uploaded);
  *ws = RescaleWs();
}

int mpp_rescale_run(hipStream_t st, RescaleWs *ws, const uint8_t *src, int H, int W, int64_t pitch, const int32_t *row_idx,
                    const double *row_w, int oh, int Tr, const int32_t *col_idx, const double *col_w, int ow, int Tc,
                    uint8_t *out, double *out_f64, int64_t ws_limit, std::string *err) {
  if (!src || !row_idx || !row_w || !col_idx || !col_w || !out) return bad(err, -1, "rescale: missing arguments");
  if (H <= 0 || W <= 0 || oh <= 0 || ow <= 0 || Tr <= 0 || Tc <= 0 || Tr > 4096 || Tc > 4096 || pitch < 3 * (int64_t)W)
    return bad(err, -1, "rescale: bad shape %d x %d (pitch %lld) -> %d x %d, %d / %d taps", H, W, (long long)pitch, oh, ow, Tr, Tc);
  if ((int64_t)ow * 3 > INT_MAX / 2 || (int64_t)oh * Tr > INT_MAX || (int64_t)ow * Tc > INT_MAX)
    return bad(err, -1, "rescale: output %d x %d too large", oh, ow);
  if (ws_limit <= 0) return bad(err, -1, "rescale: the workspace limit must be positive");

  // every index inside the image (the kernels trust the tables); the source rows each output row reads
  std::vector<int> rlo(oh), rhi(oh);
  for (int i = 0; i < oh; ++i) {
    int lo = INT_MAX, hi = -1;
    for (int t = 0; t < Tr; ++t) { const int v = row_idx[(size_t)i * Tr + t]; lo = std::min(lo, v); hi = std::max(hi, v); }
    if (lo < 0 || hi >= H) return bad(err, -1, "rescale: a row index of output row %d lies outside 0..%d", i, H - 1);
    rlo[i] = lo; rhi[i] = hi;
  }
  int span = 0;                        // widest range of source columns under the 64 output columns of one workgroup
  for (int j0 = 0; j0 < ow; j0 += RS_COLS) {
    int lo = INT_MAX, hi = -1;
    const size_t e1 = (size_t)std::min(ow, j0 + RS_COLS) * Tc;
    for (size_t e = (size_t)j0 * Tc; e < e1; ++e) { lo = std::min(lo, col_idx[e]); hi = std::max(hi, col_idx[e]); }
    if (lo < 0 || hi >= W) return bad(err, -1, "rescale: a column index of output columns %d.. lies outside 0..%d", j0, W - 1);
    span = std::max(span, hi - lo + 1);
  }
  const int row_stride = (int)(((size_t)span * 3 + 15 + 15) / 16 * 16);
  const size_t lds = (size_t)Tc * RS_COLS * 12 + 16 + (size_t)RS_ROWS * row_stride;
  if (lds > RS_LDS_MAX)
    return bad(err, -1, "rescale: %d taps over a span of %d source columns per %d output columns need %zu bytes of LDS (limit %zu)",
               Tc, span, RS_COLS, lds, RS_LDS_MAX);

  const int ow3 = ow * 3, tpitch = (ow3 + 1) & ~1;
  const size_t row_bytes = (size_t)tpitch * 8;
  const size_t off_rw = 0, off_cw = off_rw + up256((size_t)oh * Tr * 8), off_ri = off_cw + up256((size_t)ow * Tc * 8),
               off_ci = off_ri + up256((size_t)oh * Tr * 4), tab_bytes = off_ci + up256((size_t)ow * Tc * 4);
  if ((size_t)ws_limit < tab_bytes + row_bytes)
    return bad(err, -1, "rescale: the workspace limit of %lld bytes is below the tables (%zu) plus one row (%zu)",
               (long long)ws_limit, tab_bytes, row_bytes);
  // (the second bound keeps k_rescale_rows' grid within 65535 workgroups along y)
  const int64_t max_rows = std::min<int64_t>((int64_t)(((size_t)ws_limit - tab_bytes) / row_bytes), 65535 * (int64_t)RS_ROWS);

  struct Band { int i0, i1, r0, r1; };
  std::vector<Band> bands;
  int64_t band_rows = 0;
  for (int i0 = 0; i0 < oh;) {
    int lo = rlo[i0], hi = rhi[i0], i1 = i0 + 1;
    if ((int64_t)hi - lo + 1 > max_rows)
      return bad(err, -1, "rescale: output row %d alone reads %d source rows, %zu bytes of workspace; the limit is %lld", i0,
                 hi - lo + 1, tab_bytes + (size_t)(hi - lo + 1) * row_bytes, (long long)ws_limit);
    while (i1 < oh && i1 - i0 < 65535) {
      const int l2 = std::min(lo, rlo[i1]), h2 = std::max(hi, rhi[i1]);
      if ((int64_t)h2 - l2 + 1 > max_rows) break;
      lo = l2; hi = h2; ++i1;
    }
    bands.push_back({i0, i1, lo, hi + 1});
    band_rows = std::max<int64_t>(band_rows, hi - lo + 1);
    i0 = i1;
  }

  const size_t need = tab_bytes + (size_t)band_rows * row_bytes;
  if (need > ws->dev_bytes) {
    if (ws->dev) { (void)hipFree(ws->dev); ws->dev = nullptr; ws->dev_bytes = 0; }
    RS_HIP(hipMalloc((void **)&ws->dev, need));
    ws->dev_bytes = need;
  }
  if (!ws->uploaded) RS_HIP(hipEventCreateWithFlags(&ws->uploaded, hipEventDisableTiming));
  RS_HIP(hipEventSynchronize(ws->uploaded));         // (an event never recorded counts as complete)
  if (tab_bytes > ws->pin_bytes) {
    if (ws->pin) { (void)hipHostFree(ws->pin); ws->pin = nullptr; ws->pin_bytes = 0; }
    RS_HIP(hipHostMalloc((void **)&ws->pin, tab_bytes, hipHostMallocDefault));
    ws->pin_bytes = tab_bytes;
  }
  memcpy(ws->pin + off_rw, row_w, (size_t)oh * Tr * 8);
  memcpy(ws->pin + off_cw, col_w, (size_t)ow * Tc * 8);
  memcpy(ws->pin + off_ri, row_idx, (size_t)oh * Tr * 4);
  memcpy(ws->pin + off_ci, col_idx, (size_t)ow * Tc * 4);
  RS_HIP(hipMemcpyAsync(ws->dev, ws->pin, tab_bytes, hipMemcpyHostToDevice, st));
  RS_HIP(hipEventRecord(ws->uploaded, st));

  const double *d_rw = reinterpret_cast<const double *>(ws->dev + off_rw), *d_cw = reinterpret_cast<const double *>(ws->dev + off_cw);
  const int32_t *d_ri = reinterpret_cast<const int32_t *>(ws->dev + off_ri), *d_ci = reinterpret_cast<const int32_t *>(ws->dev + off_ci);
  double *tmp = reinterpret_cast<double *>(ws->dev + tab_bytes);
  const uint8_t *src_end = src + (size_t)(H - 1) * (size_t)pitch + (size_t)W * 3;
  for (const Band &b : bands) {
    const dim3 g1((unsigned)((ow + RS_COLS - 1) / RS_COLS), (unsigned)((b.r1 - b.r0 + RS_ROWS - 1) / RS_ROWS));
    hipLaunchKernelGGL(k_rescale_rows, g1, dim3(RS_THREADS), lds, st, src, src_end, (long long)pitch, b.r0, b.r1, d_ci, d_cw, ow, Tc,
                       row_stride, tmp, tpitch);
    const dim3 g2((unsigned)(((ow3 + 1) / 2 + 255) / 256), (unsigned)(b.i1 - b.i0));
    hipLaunchKernelGGL(k_rescale_cols, g2, dim3(256), 0, st, tmp, tpitch, b.r0, d_ri, d_rw, Tr, b.i0, ow3, out, out_f64);
  }
  RS_HIP(hipGetLastError());
  ws->bands = (int)bands.size();
  return 0;
}
