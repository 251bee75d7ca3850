// mpp_descent.hip -- the local descent's own device code (mpp_select_points, mpp_descend): DESIGN.md section 16.
//
//   select    one lane per point; the chain's points pass through LDS DESC_THREADS at a time and every lane that is still
//             standing tests the staged candidates for a rival with a smaller key (-value, slot) within the distance.  The
//             rule is that of mpp_select_minima on points instead of pixels: order-free, a loser's losers are dropped too;
//   remove    one workgroup per chain: the kept points leave by stable compaction in place, in ascending chunks of
//             DESC_THREADS slots.  A chunk is read whole before any of it is written and a destination never passes its
//             source, so no second copy of the state is needed.  The removed values go to a list in slot order;
//   round     one lane per chain books the round in the chain's one record, its descent report (descent_book, mpp_round.hpp);
//   summary   the largest Papangelou value of the returned state, its first slot and the count of positive ones.
// The birth half's selection and append are mpp_birth_complete.hip's, the Papangelou values k_papangelou_tiles' (mpp_scratch.hip).
#include <cmath>

#include "mpp_device.hpp"
#include "mpp_launch.hpp"
#include "mpp_round.hpp"

#define DESC_THREADS 256
#define DESC_WAVES (DESC_THREADS / WAVE)

extern "C" size_t mpp_descent_bytes(int n_chains, int cap, size_t hw) {
  const size_t T = (size_t)n_chains, TC = T * cap;
  return (3 * TC + T * hw) * sizeof(double) + T * sizeof(mpp_descent_report) + (TC + T) * sizeof(int32_t) + TC;
}
// (the doubles first, then the records, the ints, the bytes: every array is aligned for its type)
extern "C" void mpp_descent_plan(Descent *d, int n_chains, int cap, size_t hw, void *ws) {
  const size_t T = (size_t)n_chains, TC = T * cap;
  d->n_chains = n_chains; d->cap = cap;
  d->p = (double *)ws; d->rem_val = d->p + TC; d->gain_val = d->rem_val + TC;
  d->dE = hw ? d->gain_val + TC : nullptr;
  d->rep = (mpp_descent_report *)(d->gain_val + TC + T * hw);
  d->src = (int32_t *)(d->rep + T);
  d->n_rem = d->src + TC;
  d->keep = (uint8_t *)(d->n_rem + T);
}

__device__ __forceinline__ int desc_count(const TileRef &t, int cap) {
  const int n = *t.n;
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// ---- the selection among points ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DESC_THREADS) void k_ptsel(PtSel s) {
  __shared__ int s_x[DESC_THREADS], s_y[DESC_THREADS];
  __shared__ double s_v[DESC_THREADS];
  const int chain = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int32_t *x = s.x, *y = s.y;
  int stride = s.stride, n = s.n;
  if (s.tiles) {
    const TileRef t = s.tiles[chain];
    x = t.px; y = t.py; stride = 1;
    n = (s.closed && s.closed[chain].status >= 0) ? 0 : desc_count(t, s.cap);
  }
  if ((long long)blockIdx.x * DESC_THREADS >= n) return;        // (the whole block alike)
  const double *val = s.val + (size_t)chain * s.pitch;
  const int i = blockIdx.x * DESC_THREADS + tid;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double v = nan;
  long long xi = 0, yi = 0;
  bool cand = false;
  if (i < n) {
    v = val[i];
    cand = v > s.above;                                          // (false for a NaN, true for +inf)
    xi = x[(size_t)i * stride]; yi = y[(size_t)i * stride];
  }
  bool keep = cand;
  for (int base = 0; base < n; base += DESC_THREADS) {
    const int j = base + tid;
    __syncthreads();                                             // (the staged chunk has been read by every lane)
    double vj = nan;
    if (j < n) {
      const double w = val[j];
      vj = w > s.above ? w : nan;                                // a point that is no candidate beats nobody: a NaN compares false
      s_x[tid] = x[(size_t)j * stride]; s_y[tid] = y[(size_t)j * stride];
    }
    s_v[tid] = vj;
    __syncthreads();
    if (keep) {
      const int m = n - base < DESC_THREADS ? n - base : DESC_THREADS;
      for (int k = 0; k < m; ++k) {
        const double v2 = s_v[k];
        if (!(v2 > v || (v2 == v && base + k < i))) continue;    // (itself: equal value, equal slot)
        const long long dx = (long long)s_x[k] - xi, dy = (long long)s_y[k] - yi;
        if ((double)(dx * dx + dy * dy) <= s.d2) { keep = false; break; }
      }
    }
  }
  if (i < n) s.keep[(size_t)chain * s.pitch + i] = keep ? 1 : 0;
  if (s.count) {
    const unsigned long long mc = __ballot(cand), mk = __ballot(keep);
    if (lane == 0) {
      if (mc) atomicAdd(&s.count[0], __popcll(mc));
      if (mk) atomicAdd(&s.count[1], __popcll(mk));
    }
  }
}

// ---- the descent -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DESC_THREADS) void k_descent_init(const TileRef *tiles, Descent d) {
  const int chain = blockIdx.x, tid = threadIdx.x;
  const int n = desc_count(tiles[chain], d.cap);
  int32_t *src = d.src + (size_t)chain * d.cap;
  for (int i = tid; i < d.cap; i += DESC_THREADS) src[i] = i < n ? i : -1;
  if (tid != 0) return;
  mpp_descent_report r{};                                        // (the counts and the gains start at 0)
  r.status = -1; r.n_after = n; r.slot_max = -1; r.max_p = -HUGE_VAL; r.x = -1; r.y = -1;
  d.rep[chain] = r;
  d.n_rem[chain] = 0;
}

// The points the selection kept leave an open chain; the survivors keep their order.  rem_val[chain][place]: the removed
// values in slot order; n_rem[chain]: their number.  The count and the error code are written only when a point left.
__global__ __launch_bounds__(DESC_THREADS) void k_descent_remove(const TileRef *tiles, Descent d) {
  // (two predicates scanned behind one pair of barriers: block_scan_place, mpp_device.hpp, twice would take two pairs)
  __shared__ int s_s[DESC_WAVES], s_r[DESC_WAVES];
  const int chain = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  if (d.rep[chain].status >= 0) return;                          // (closed: not touched again)
  TileRef t = tiles[chain];
  const int n = desc_count(t, d.cap);
  const size_t o = (size_t)chain * d.cap;
  const uint8_t *gone_of = d.keep + o;
  const double *p = d.p + o;
  int32_t *src = d.src + o;
  double *rem_val = d.rem_val + o;
  const unsigned long long lower = (1ull << lane) - 1ull;
  int n_stay = 0, n_gone = 0;
  for (int base = 0; base < n; base += DESC_THREADS) {
    const int i = base + tid;
    const bool in = i < n, gone = in && gone_of[i] != 0, stay = in && !gone;
    int px = 0, py = 0, from = -1;
    double ps = 0.0, pr = 0.0, pa = 0.0, pv = 0.0;
    if (stay) { px = t.px[i]; py = t.py[i]; ps = t.ps[i]; pr = t.pr[i]; pa = t.pa[i]; from = src[i]; }
    if (gone) pv = p[i];
    const unsigned long long ms = __ballot(stay), mg = __ballot(gone);
    if (lane == 0) { s_s[wave] = __popcll(ms); s_r[wave] = __popcll(mg); }
    __syncthreads();                                             // (the chunk has been read whole)
    int at_s = n_stay + __popcll(ms & lower), at_g = n_gone + __popcll(mg & lower), tot_s = 0, tot_g = 0;
#pragma unroll
    for (int w = 0; w < DESC_WAVES; ++w) {
      at_s += w < wave ? s_s[w] : 0; at_g += w < wave ? s_r[w] : 0;
      tot_s += s_s[w]; tot_g += s_r[w];
    }
    if (stay && at_s != i) {                                     // (at_s <= i: a destination never passes its source)
      t.px[at_s] = px; t.py[at_s] = py; t.ps[at_s] = ps; t.pr[at_s] = pr; t.pa[at_s] = pa; src[at_s] = from;
    }
    if (gone) rem_val[at_g] = pv;                                // (at_g < n <= cap)
    __syncthreads();                                             // (the wave counts may be overwritten)
    n_stay += tot_s; n_gone += tot_g;
  }
  for (int i = n_stay + tid; i < n; i += DESC_THREADS) src[i] = -1;
  if (tid == 0) {
    d.n_rem[chain] = n_gone;
    if (n_gone > 0) { *t.n = n_stay; *t.err = 0; }               // (what mpp_set_points of the survivors leaves)
  }
}

// one lane per chain: the round's book.  n_kept: nullptr, or the candidates the birth half kept per chain (MinSel::n_kept)
__global__ __launch_bounds__(WAVE) void k_descent_round(const TileRef *tiles, Descent d, int what, int max_rounds, const int32_t *n_kept) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.n_chains || d.rep[c].status >= 0) return;
  mpp_descent_report r = d.rep[c];
  const size_t o = (size_t)c * d.cap;
  descent_book(r, what, max_rounds, d.cap, tiles[c].n, tiles[c].err, d.n_rem[c], d.rem_val + o, n_kept ? n_kept[c] : 0, d.gain_val + o);
  d.rep[c] = r;
}

// max_p, slot_max, n_positive of every chain's state from d.p (nullptr: skipped); the map's summary is copied in when there is one
__global__ __launch_bounds__(DESC_THREADS) void k_descent_summary(const TileRef *tiles, Descent d, const mpp_birth_summary *sum) {
  __shared__ double s_v[DESC_THREADS];
  __shared__ int s_i[DESC_THREADS], s_c[DESC_THREADS];
  const int chain = blockIdx.x, tid = threadIdx.x;
  const int n = d.p ? desc_count(tiles[chain], d.cap) : 0;
  const double *p = d.p + (size_t)chain * d.cap;
  double best = -HUGE_VAL;
  int slot = -1, pos = 0;
  for (int i = tid; i < n; i += DESC_THREADS) {                  // (ascending: the first of equal values stays)
    const double v = p[i];
    pos += v > 0.0 ? 1 : 0;
    if (v == v && (slot < 0 || v > best)) { best = v; slot = i; }
  }
  s_v[tid] = best; s_i[tid] = slot; s_c[tid] = pos;
  __syncthreads();
  for (int h = DESC_THREADS / 2; d.p && h > 0; h >>= 1) {
    if (tid < h) {
      const double v2 = s_v[tid + h];
      const int i2 = s_i[tid + h];
      if (i2 >= 0 && (s_i[tid] < 0 || v2 > s_v[tid] || (v2 == s_v[tid] && i2 < s_i[tid]))) { s_v[tid] = v2; s_i[tid] = i2; }
      s_c[tid] += s_c[tid + h];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  mpp_descent_report *r = d.rep + chain;
  r->max_p = s_v[0]; r->slot_max = s_i[0]; r->n_positive = s_c[0];  // ((-inf, -1, 0) without d.p, as k_descent_init wrote them)
  if (sum) {
    const mpp_birth_summary b = sum[chain];
    r->min_dE = b.min_dE; r->x = b.x; r->y = b.y; r->n_negative = b.n_negative; r->n_nan = b.n_nan;
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
extern "C" void mpp_launch_ptsel(hipStream_t st, const PtSel &s) {
  const int n = s.tiles ? s.cap : s.n, chains = s.tiles ? s.n_chains : 1;
  if (n <= 0 || chains <= 0) return;
  hipLaunchKernelGGL(k_ptsel, dim3((n + DESC_THREADS - 1) / DESC_THREADS, chains), dim3(DESC_THREADS), 0, st, s);
}
extern "C" void mpp_launch_descent_init(hipStream_t st, const TileRef *tiles, const Descent &d) {
  if (d.n_chains <= 0) return;
  hipLaunchKernelGGL(k_descent_init, dim3(d.n_chains), dim3(DESC_THREADS), 0, st, tiles, d);
}
extern "C" void mpp_launch_descent_remove(hipStream_t st, const TileRef *tiles, const Descent &d) {
  if (d.n_chains <= 0) return;
  hipLaunchKernelGGL(k_descent_remove, dim3(d.n_chains), dim3(DESC_THREADS), 0, st, tiles, d);
}
extern "C" void mpp_launch_descent_round(hipStream_t st, const TileRef *tiles, const Descent &d, int what, int max_rounds, const int32_t *n_kept) {
  if (d.n_chains <= 0) return;
  hipLaunchKernelGGL(k_descent_round, dim3((d.n_chains + WAVE - 1) / WAVE), dim3(WAVE), 0, st, tiles, d, what, max_rounds, n_kept);
}
extern "C" void mpp_launch_descent_summary(hipStream_t st, const TileRef *tiles, const Descent &d, const mpp_birth_summary *sum) {
  if (d.n_chains <= 0) return;
  hipLaunchKernelGGL(k_descent_summary, dim3(d.n_chains), dim3(DESC_THREADS), 0, st, tiles, d, sum);
}
