// mpp_detect.hip -- detection step of the CNN-only baseline (PosNet centres, ShapeNet marks) on a whole score map.
//
//  * threshold + greedy distance NMS (pos_net_model.py:376-380, shape_net_model.py:285-288, utils/nms.py:68-110) as the
//    lexicographically-first independent set of the candidates under the "within nms_distance" relation, decided in
//    parallel rounds on the pixel grid (the map is its own spatial hash: nothing is sorted before the NMS);
//  * the argmax class (first maximum, np.argmax) of the three mark maps at a list of pixels
//    (output_vector_to_value, models/shape_net/mappings.py:145-157).
//
// Rank of a candidate: its value, ties toward the larger row-major flat index (the convention of k_naive_init and the
// oracle).  A candidate is KEPT iff every candidate ranked above it within the radius is REMOVED, REMOVED iff one of them
// is KEPT; both transitions are final, so by induction on rank the fixpoint is the greedy walk's result.  One workgroup
// holds a 64 x 64 tile plus a halo of floor(nms_distance) in LDS, iterates to its local fixpoint and writes back its
// interior only; the host relaunches while candidates are undecided.  A stale halo read only delays a decision, and the
// top-ranked undecided candidate always decides, so every launch makes progress.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>

#include "mpp_detect.hpp"
#include "mpp_rank_key.hpp"

namespace {

enum : uint8_t { ST_NONE = 0, ST_UNDEC = 1, ST_KEPT = 2, ST_REMOVED = 3 };
constexpr int TILE = 64;
constexpr int RES_THREADS = 256;

// state of every pixel, the candidate count, and a flag per 64 x 64 tile that holds a candidate
__global__ __launch_bounds__(256) void k_detect_init(const float *det, int H, int W, int ld, float thr, int strict, uint8_t *state,
                                                     uint8_t *tile_flag, int ntx, unsigned long long *n_cand) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  int cnt = 0;
  for (int r = blockIdx.y * 4 + threadIdx.y; r < H; r += gridDim.y * 4) {
    if (c >= W) break;
    const float v = det[(size_t)r * ld + c];
    const bool cand = strict ? (v > thr) : (v >= thr);       // float32 compare, as NumPy does float32 array vs float
    state[(size_t)r * W + c] = cand ? ST_UNDEC : ST_NONE;
    if (cand) {
      ++cnt;
      tile_flag[(size_t)(r / TILE) * ntx + c / TILE] = 1;
    }
  }
  // per-wave sum, one atomic per wave
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_cand, (unsigned long long)cnt);
}

// One resolve round of every tile that still holds undecided candidates.  LDS: the ordered values and states of the tile
// and its halo (S x S, S = 64 + 2R), and the half-width of the disk per row offset.
__global__ __launch_bounds__(RES_THREADS) void k_detect_resolve(const float *det, int H, int W, int ld, uint8_t *state,
                                                                uint8_t *tile_flag, int ntx, int R, double nms_d,
                                                                unsigned long long *n_undec) {
  extern __shared__ uint32_t lds[];
  __shared__ int halfw[2 * 32 + 1];
  const int tile = blockIdx.x;
  if (!tile_flag[tile]) return;
  const int S = TILE + 2 * R;
  uint32_t *val = lds;
  uint8_t *st = (uint8_t *)(lds + S * S);
  const int r0 = (tile / ntx) * TILE, c0 = (tile % ntx) * TILE;
  // disk rows: |dy| <= halfw[dx + R]  <=>  !(sqrt(dx^2 + dy^2) > nms_d)  (utils/nms.py:103-105, in double)
  if ((int)threadIdx.x <= 2 * R) {
    const int dx = (int)threadIdx.x - R;
    int w = -1;
    for (int dy = 0; dy <= R; ++dy)
      if (!(sqrt((double)(dx * dx + dy * dy)) > nms_d)) w = dy;
    halfw[threadIdx.x] = w;
  }
  for (int i = threadIdx.x; i < S * S; i += RES_THREADS) {
    const int gr = r0 - R + i / S, gc = c0 - R + i % S;
    uint8_t s = ST_NONE;
    uint32_t v = 0;
    if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
      s = state[(size_t)gr * W + gc];
      if (s != ST_NONE) v = ordered_bits(det[(size_t)gr * ld + gc]);
    }
    val[i] = v;
    st[i] = s;
  }
  __syncthreads();
  const int ic = threadIdx.x % TILE, ir0 = threadIdx.x / TILE;
  constexpr int ROWS_PER_PASS = RES_THREADS / TILE;
  while (true) {
    int changed = 0;
    for (int ir = ir0; ir < TILE; ir += ROWS_PER_PASS) {
      const int p = (ir + R) * S + ic + R;
      if (st[p] != ST_UNDEC) continue;        // (pixels outside the map are NONE)
      const uint32_t mv = val[p];
      bool kill = false, wait = false;
      for (int dx = -R; dx <= R && !kill; ++dx) {
        const int w = halfw[dx + R];
        for (int dy = -w; dy <= w; ++dy) {
          const int q = p + dx * S + dy;
          const uint8_t s = st[q];
          if (s == ST_NONE || s == ST_REMOVED) continue;
          const uint32_t qv = val[q];
          // ranked above p: larger value, or the same value and a larger flat index (row-major: dx > 0, or dx == 0, dy > 0)
          if (qv > mv || (qv == mv && (dx > 0 || (dx == 0 && dy > 0)))) {
            if (s == ST_KEPT) { kill = true; break; }
            wait = true;
          }
        }
      }
      if (kill) { st[p] = ST_REMOVED; changed = 1; }
      else if (!wait) { st[p] = ST_KEPT; changed = 1; }
    }
    if (!__syncthreads_or(changed)) break;
  }
  int undec = 0;
  for (int ir = ir0; ir < TILE; ir += ROWS_PER_PASS) {
    const int gr = r0 + ir, gc = c0 + ic;
    if (gr >= H || gc >= W) continue;
    const uint8_t s = st[(ir + R) * S + ic + R];
    if (s == ST_NONE) continue;
    state[(size_t)gr * W + gc] = s;
    undec += s == ST_UNDEC;
  }
  undec = __syncthreads_count(undec > 0);
  if (threadIdx.x == 0) {
    if (undec) atomicAdd(n_undec, 1ull);     // (tiles with undecided candidates; the count of tiles is what the host needs)
    else tile_flag[tile] = 0;
  }
}

// keys (ordered value << 32 | flat index) of the kept pixels, in no particular order
__global__ __launch_bounds__(256) void k_detect_compact(const float *det, int H, int W, int ld, const uint8_t *state,
                                                        unsigned long long *keys, unsigned long long cap, unsigned long long *n_kept) {
  const size_t hw = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (size_t)gridDim.x * blockDim.x) {
    if (state[i] != ST_KEPT) continue;
    const int r = (int)(i / W), c = (int)(i % W);
    const unsigned long long k = atomicAdd(n_kept, 1ull);
    if (k < cap) keys[k] = ((unsigned long long)ordered_bits(det[(size_t)r * ld + c]) << 32) | (unsigned long long)i;
  }
}

__global__ __launch_bounds__(256) void k_detect_decode(const float *det, int W, int ld, const unsigned long long *keys, int n,
                                                       int32_t *xy, float *scores) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned int flat = (unsigned int)(keys[i] & 0xffffffffull);
  const int r = (int)(flat / (unsigned)W), c = (int)(flat % (unsigned)W);
  xy[2 * i] = r;
  xy[2 * i + 1] = c;
  scores[i] = det[(size_t)r * ld + c];
}

// argmax class (first maximum; a NaN wins as in np.argmax) of the three mark maps at n pixels; a pixel outside the map: -1
__global__ __launch_bounds__(256) void k_mark_classes(int H, int W, int ld, const float *m0, const float *m1, const float *m2, int n,
                                                      const int32_t *xy, int32_t *classes) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t / 3, k = t % 3;
  if (i >= n) return;
  const int r = xy[2 * i], c = xy[2 * i + 1];
  int am = -1;
  if (r >= 0 && r < H && c >= 0 && c < W) {
    const float *row = (k == 0 ? m0 : k == 1 ? m1 : m2) + ((size_t)r * ld + c) * 32;
    am = 0;
    float best = row[0];
    if (!isnan(best))
      for (int j = 1; j < 32; ++j) {
        const float v = row[j];
        if (isnan(v)) { am = j; break; }
        if (v > best) { best = v; am = j; }
      }
  }
  classes[3 * i + k] = am;
}

template <typename T>
hipError_t grow(T **p, size_t *have, size_t want) {
  if (*p && *have >= want) return hipSuccess;
  if (*p) { (void)hipFree(*p); *p = nullptr; *have = 0; }
  hipError_t e = hipMalloc((void **)p, want ? want * sizeof(T) : sizeof(T));
  if (e == hipSuccess) *have = want;
  return e;
}

int failf(std::string *err, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
int failf(std::string *err, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (err) *err = buf;
  return code;
}

}  // namespace

#define DCHK(call)                                                                                 \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) return failf(err, -2, "%s failed: %s", #call, hipGetErrorString(e_));    \
  } while (0)

void mpp_detect_free(DetectWs *ws) {
  if (ws->state) (void)hipFree(ws->state);
  if (ws->tile_flag) (void)hipFree(ws->tile_flag);
  if (ws->counters) (void)hipFree(ws->counters);
  if (ws->keys) (void)hipFree(ws->keys);
  if (ws->sort_tmp) (void)hipFree(ws->sort_tmp);
  *ws = DetectWs();
}

int mpp_detect_run(hipStream_t st, DetectWs *ws, int H, int W, int ld, const float *det, double threshold, int strict,
                   double nms_distance, int cap, int32_t *xy, float *scores, int64_t *n_candidates, int64_t *n_kept,
                   std::string *err) {
  ws->launches = 0;
  if (H < 0 || W < 0 || (H > 0 && W > 0 && (!det || ld < W)) || cap < 0 || (cap > 0 && (!xy || !scores)) || !n_candidates || !n_kept)
    return failf(err, -1, "detect_centers: bad arguments (H %d, W %d, ld %d, cap %d)", H, W, ld, cap);
  if ((long long)H * W >= (1ll << 31))
    return failf(err, -1, "detect_centers: a %d x %d map has 2^31 pixels or more (flat indices are 31-bit); split it", H, W);
  if (!(nms_distance >= 0.0 && nms_distance <= MPP_DETECT_MAX_NMS))
    return failf(err, -1, "detect_centers: nms_distance %g outside [0, %g] (the halo of a tile)", nms_distance, MPP_DETECT_MAX_NMS);
  *n_candidates = *n_kept = 0;
  if ((long long)H * W == 0) return 0;
  const size_t hw = (size_t)H * W;
  const int ntx = (W + TILE - 1) / TILE, nty = (H + TILE - 1) / TILE;
  const size_t n_tiles = (size_t)ntx * nty;
  size_t have3 = ws->counters ? 3 : 0;
  DCHK(grow(&ws->state, &ws->state_bytes, hw));
  DCHK(grow(&ws->tile_flag, &ws->flag_bytes, n_tiles));
  DCHK(grow(&ws->counters, &have3, (size_t)3));
  DCHK(hipMemsetAsync(ws->tile_flag, 0, n_tiles, st));
  DCHK(hipMemsetAsync(ws->counters, 0, 3 * sizeof(unsigned long long), st));
  const int gy = (int)std::min<long long>((H + 3) / 4, 16384);
  hipLaunchKernelGGL(k_detect_init, dim3(ntx, gy), dim3(64, 4), 0, st, det, H, W, ld, (float)threshold, strict, ws->state,
                     ws->tile_flag, ntx, ws->counters);
  DCHK(hipGetLastError());
  unsigned long long h[3] = {0, 0, 0};
  DCHK(hipMemcpyAsync(h, ws->counters, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  DCHK(hipStreamSynchronize(st));
  const unsigned long long n_cand = h[0];
  *n_candidates = (int64_t)n_cand;
  if (n_cand == 0) return 0;

  const int R = (int)std::floor(nms_distance);
  const int S = TILE + 2 * R;
  const size_t lds = (size_t)S * S * (sizeof(uint32_t) + 1);
  DCHK(hipFuncSetAttribute((const void *)k_detect_resolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  unsigned long long undec_tiles = n_tiles;
  // every launch decides at least the top-ranked undecided candidate: more launches than candidates is a bug, not a retry
  while (true) {
    if ((unsigned long long)ws->launches >= n_cand)
      return failf(err, -9, "detect_centers: %llu candidates still undecided in %llu tiles after %d resolve launches",
                   n_cand, undec_tiles, ws->launches);
    DCHK(hipMemsetAsync(ws->counters + 1, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_detect_resolve, dim3((unsigned)n_tiles), dim3(RES_THREADS), lds, st, det, H, W, ld, ws->state,
                       ws->tile_flag, ntx, R, nms_distance, ws->counters + 1);
    DCHK(hipGetLastError());
    ++ws->launches;
    DCHK(hipMemcpyAsync(&h[1], ws->counters + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    DCHK(hipStreamSynchronize(st));
    undec_tiles = h[1];
    if (undec_tiles == 0) break;
  }

  DCHK(grow(&ws->keys, &ws->key_count, 2 * (size_t)n_cand));
  unsigned long long *keys_in = ws->keys, *keys_out = ws->keys + n_cand;
  const int gc = (int)std::min<size_t>((hw + 255) / 256, 8192);
  hipLaunchKernelGGL(k_detect_compact, dim3(gc), dim3(256), 0, st, det, H, W, ld, ws->state, keys_in, n_cand, ws->counters + 2);
  DCHK(hipGetLastError());
  DCHK(hipMemcpyAsync(&h[2], ws->counters + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  DCHK(hipStreamSynchronize(st));
  const unsigned long long kept = h[2];
  *n_kept = (int64_t)kept;
  if (kept > n_cand) return failf(err, -9, "detect_centers: %llu kept of %llu candidates", kept, n_cand);
  if (kept > (unsigned long long)cap)
    return failf(err, MPP_DETECT_E_FULL, "detect_centers: %llu centres kept, the output holds %d", kept, cap);
  if (kept == 0) return 0;
  size_t tmp_need = 0;
  DCHK(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, tmp_need, keys_in, keys_out, (int)kept, 0, 64, st));
  DCHK(grow(&ws->sort_tmp, &ws->sort_tmp_bytes, tmp_need));
  size_t tmp_bytes = ws->sort_tmp_bytes;
  DCHK(hipcub::DeviceRadixSort::SortKeysDescending(ws->sort_tmp, tmp_bytes, keys_in, keys_out, (int)kept, 0, 64, st));
  hipLaunchKernelGGL(k_detect_decode, dim3((unsigned)((kept + 255) / 256)), dim3(256), 0, st, det, W, ld, keys_out, (int)kept, xy,
                     scores);
  DCHK(hipGetLastError());
  return 0;
}

void mpp_launch_mark_classes(hipStream_t st, int H, int W, int ld, const float *m0, const float *m1, const float *m2, int n,
                             const int32_t *xy, int32_t *classes) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_mark_classes, dim3((unsigned)((3ll * n + 255) / 256)), dim3(256), 0, st, H, W, ld, m0, m1, m2, n, xy, classes);
}
