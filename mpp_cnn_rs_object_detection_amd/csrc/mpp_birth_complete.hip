// mpp_birth_complete.hip -- the selection of a map's local minima (mpp_select_minima) and the append of the kept ones, the birth
// half of a round of mpp_birth_complete and mpp_descend (the round's book is k_descent_round's): DESIGN.md section 13.
//
//   candidates  the pixels with dE < below, compacted by ballot into a list in row-major order: a count per block of
//               MINSEL_SPAN pixels, an exclusive scan of the counts, the same ballots again to fill;
//   resolve     one lane per candidate.  The list is sorted by pixel, so the candidates of a row are a contiguous run (its
//               start found once per row by bisection) and those within reach of a column a sub-run: a candidate walks the
//               runs of the rows within floor(distance) of its own and stops at the first candidate with a smaller key.  The
//               list lives in device memory: it may hold every pixel of the map;
//   output      the kept candidates keep the list's order: their count per block of the resolve, a scan, and a kernel that
//               writes each to its place -- the caller's arrays (mpp_select_minima), or the slots behind a chain's
//               configuration with the candidate's marks (the completion).
#include "mpp_birth.hpp"
#include "mpp_device.hpp"
#include "mpp_launch.hpp"

#define MINSEL_THREADS 256
#define MINSEL_WAVES (MINSEL_THREADS / WAVE)
#define MINSEL_ITEMS 8
#define MINSEL_SPAN (MINSEL_THREADS * MINSEL_ITEMS)     // pixels per block of the compaction

static int minsel_blocks(long long hw, int per) { return (int)((hw + per - 1) / per); }

extern "C" size_t mpp_minsel_bytes(int n_chains, int H, int W) {
  const size_t T = (size_t)n_chains, hw = (size_t)H * W;
  const size_t ints = T * (hw + (size_t)H + 1 + minsel_blocks(hw, MINSEL_SPAN) + minsel_blocks(hw, MINSEL_THREADS) + 2);
  return T * hw * sizeof(double) + ints * sizeof(int32_t) + T * hw;
}
// (the doubles first, then the ints, then the bytes: every array is aligned for its type)
extern "C" void mpp_minsel_plan(MinSel *s, void *ws) {
  const size_t T = (size_t)s->n_chains, hw = (size_t)s->H * s->W;
  s->nb_fill = minsel_blocks(hw, MINSEL_SPAN); s->nb_res = minsel_blocks(hw, MINSEL_THREADS);
  s->val = (double *)ws;
  s->idx = (int32_t *)(s->val + T * hw);
  s->rows = s->idx + T * hw;
  s->cblk = s->rows + T * ((size_t)s->H + 1);
  s->kblk = s->cblk + T * s->nb_fill;
  s->n_cand = s->kblk + T * s->nb_res;
  s->n_kept = s->n_cand + T;
  s->keep = (uint8_t *)(s->n_kept + T);
}

__device__ __forceinline__ bool minsel_closed(const MinSel &s, int chain) { return s.rep && s.rep[chain].status >= 0; }

// ---- the candidates: count per block, then fill in row-major order ---------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(MINSEL_THREADS) void k_minsel_compact(MinSel s) {
  __shared__ int s_w[MINSEL_WAVES];
  const int chain = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const long long hw = (long long)s.H * s.W;
  const double *d = s.dE + (size_t)chain * s.chain_stride;
  const bool closed = minsel_closed(s, chain);                 // (a closed chain of the descent has no candidates)
  const size_t lbase = (size_t)chain * hw;
  int at = FILL ? s.cblk[(size_t)chain * s.nb_fill + blockIdx.x] : 0;      // (after the scan: where this block's run starts)
  int mine = 0;
  for (int it = 0; it < MINSEL_ITEMS; ++it) {
    const long long p = (long long)blockIdx.x * MINSEL_SPAN + it * MINSEL_THREADS + tid;
    double v = 0.0;
    bool is = false;
    if (p < hw && !closed) {
      const int x = (int)(p / s.W), y = (int)(p - (long long)x * s.W);
      v = d[(size_t)x * s.ld + y];
      is = v < s.below;                                        // (false for a NaN, true for -inf)
    }
    if (!FILL) {
      const unsigned long long m = __ballot(is);
      mine += lane == 0 ? __popcll(m) : 0;
      continue;
    }
    int total;
    const int pos = at + block_scan_place<MINSEL_WAVES>(is, s_w, &total);
    if (is) { s.idx[lbase + pos] = (int32_t)p; s.val[lbase + pos] = v; }    // (pos < the chain's candidates <= hw)
    at += total;
  }
  if (!FILL) {
    if (lane == 0) s_w[wave] = mine;
    __syncthreads();
    if (tid == 0) {
      int c = 0;
      for (int w = 0; w < MINSEL_WAVES; ++w) c += s_w[w];
      s.cblk[(size_t)chain * s.nb_fill + blockIdx.x] = c;
    }
  }
}

// exclusive scan of a chain's nblk block counts, in place; the sum goes to total[chain]
__global__ __launch_bounds__(MINSEL_THREADS) void k_minsel_scan(int32_t *blk, int nblk, int32_t *total) {
  __shared__ int sh[MINSEL_THREADS];
  const int chain = blockIdx.x, tid = threadIdx.x;
  int32_t *b = blk + (size_t)chain * nblk;
  int carry = 0;
  for (int base = 0; base < nblk; base += MINSEL_THREADS) {
    const int i = base + tid, v = i < nblk ? b[i] : 0;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < MINSEL_THREADS; d <<= 1) {
      const int add = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    if (i < nblk) b[i] = carry + sh[tid] - v;
    carry += sh[MINSEL_THREADS - 1];
    __syncthreads();
  }
  if (tid == 0) total[chain] = carry;
}

// rows[x] = the first entry of the chain's list at or behind pixel (x, 0), x = 0 .. H (rows[H] = the list's length)
__global__ __launch_bounds__(MINSEL_THREADS) void k_minsel_rows(MinSel s) {
  const int chain = blockIdx.y, x = blockIdx.x * MINSEL_THREADS + threadIdx.x;
  if (x > s.H) return;
  const int32_t *idx = s.idx + (size_t)chain * s.H * s.W;
  const long long key = (long long)x * s.W;
  int lo = 0, hi = s.n_cand[chain];
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (idx[mid] < key) lo = mid + 1; else hi = mid;
  }
  s.rows[(size_t)chain * (s.H + 1) + x] = lo;
}

// ---- resolve: kept iff no other candidate within the distance has a smaller key ------------------------------------------------
__global__ __launch_bounds__(MINSEL_THREADS) void k_minsel_resolve(MinSel s) {
  __shared__ int s_w[MINSEL_WAVES];
  const int chain = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int n = s.n_cand[chain], i = blockIdx.x * MINSEL_THREADS + tid;
  const size_t lbase = (size_t)chain * s.H * s.W;
  const int32_t *idx = s.idx + lbase;
  const double *val = s.val + lbase;
  const int32_t *rows = s.rows + (size_t)chain * (s.H + 1);
  bool keep = false;
  if (i < n) {
    keep = true;
    const int id = idx[i], x = id / s.W, y = id - x * s.W, r = s.reach;
    const double v = val[i];
    const int x_lo = x - r < 0 ? 0 : x - r, x_hi = x + r > s.H - 1 ? s.H - 1 : x + r;
    const int y_lo = y - r < 0 ? 0 : y - r, y_hi = y + r > s.W - 1 ? s.W - 1 : y + r;
    for (int xx = x_lo; xx <= x_hi && keep; ++xx) {
      int lo = rows[xx];
      const int end = rows[xx + 1];
      if (lo == end) continue;
      const int first = xx * s.W + y_lo, last = xx * s.W + y_hi;
      int hi = end;
      while (lo < hi) {                                        // the row's first candidate at or behind column y_lo
        const int mid = lo + (hi - lo) / 2;
        if (idx[mid] < first) lo = mid + 1; else hi = mid;
      }
      const long long dx = xx - x;
      for (int j = lo; j < end; ++j) {
        const int id2 = idx[j];
        if (id2 > last) break;
        if (id2 == id) continue;
        const long long dy = (id2 - xx * s.W) - y;
        if ((double)(dx * dx + dy * dy) > s.d2) continue;
        const double v2 = val[j];
        if (v2 < v || (v2 == v && id2 < id)) { keep = false; break; }
      }
    }
    s.keep[lbase + i] = keep ? 1 : 0;
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) s_w[wave] = __popcll(m);
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int w = 0; w < MINSEL_WAVES; ++w) c += s_w[w];
    s.kblk[(size_t)chain * s.nb_res + blockIdx.x] = c;
  }
}

// The place of this lane's candidate among the chain's kept ones, -1 if it is none or not kept; *id, *v: the candidate.
// Every lane of the block calls it (it synchronises); s_w: MINSEL_WAVES ints of LDS.
__device__ __forceinline__ int minsel_kept_place(const MinSel &s, int chain, int *s_w, int *id, double *v) {
  const int i = blockIdx.x * MINSEL_THREADS + threadIdx.x;
  const size_t lbase = (size_t)chain * s.H * s.W;
  const bool kept = i < s.n_cand[chain] && s.keep[lbase + i] != 0;
  if (kept) { *id = s.idx[lbase + i]; *v = s.val[lbase + i]; }
  int total;                                                   // (not needed: the block's start comes from the scan of kblk)
  const int pos = s.kblk[(size_t)chain * s.nb_res + blockIdx.x] + block_scan_place<MINSEL_WAVES, false>(kept, s_w, &total);
  return kept ? pos : -1;
}

// mpp_select_minima's output: out_cap >= the chain's kept count (the host has checked)
__global__ __launch_bounds__(MINSEL_THREADS) void k_minsel_emit(MinSel s, int out_cap, int32_t *xy, double *values) {
  __shared__ int s_w[MINSEL_WAVES];
  int id = 0;
  double v = 0.0;
  const int pos = minsel_kept_place(s, blockIdx.y, s_w, &id, &v);
  if (pos < 0 || pos >= out_cap) return;
  const size_t o = (size_t)blockIdx.y * out_cap + pos;
  xy[2 * o] = id / s.W; xy[2 * o + 1] = id % s.W;
  values[o] = v;
}

// ---- the completion ----------------------------------------------------------------------------------------------------------
// The kept candidates of an open chain go behind its configuration, slot n + place, when all of them fit; their values go to
// gain_val [n_chains][cap] by place, for the sum k_descent_round forms.  The count itself is k_descent_round's to change.
__global__ __launch_bounds__(MINSEL_THREADS) void k_complete_append(MinSel s, const DevParams *P, const TileRef *tiles, int cap,
                                                                    double *gain_val) {
  __shared__ int s_w[MINSEL_WAVES];
  const int chain = blockIdx.y;
  int id = 0;
  double v = 0.0;
  const int pos = minsel_kept_place(s, chain, s_w, &id, &v);
  if (pos < 0 || minsel_closed(s, chain)) return;
  TileRef t = tiles[chain];
  const int n = *t.n, k = s.n_kept[chain];
  if (n < 0 || k > cap - n) return;                            // (status 2: nothing of this round is appended)
  const int x = id / s.W, y = id - x * s.W, slot = n + pos;    // (pos < k: slot < cap)
  double ms, mr, ma;
  birth_candidate_marks(P, t, x, y, s.W, &ms, &mr, &ma);
  t.px[slot] = x; t.py[slot] = y; t.ps[slot] = ms; t.pr[slot] = mr; t.pa[slot] = ma;
  gain_val[(size_t)chain * cap + pos] = v;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
extern "C" void mpp_launch_minsel(hipStream_t st, const MinSel &s) {
  if (s.n_chains <= 0) return;
  const dim3 fill(s.nb_fill, s.n_chains), res(s.nb_res, s.n_chains);
  hipLaunchKernelGGL(k_minsel_compact<false>, fill, dim3(MINSEL_THREADS), 0, st, s);
  hipLaunchKernelGGL(k_minsel_scan, dim3(s.n_chains), dim3(MINSEL_THREADS), 0, st, s.cblk, s.nb_fill, s.n_cand);
  hipLaunchKernelGGL(k_minsel_compact<true>, fill, dim3(MINSEL_THREADS), 0, st, s);
  hipLaunchKernelGGL(k_minsel_rows, dim3((s.H + 1 + MINSEL_THREADS - 1) / MINSEL_THREADS, s.n_chains), dim3(MINSEL_THREADS), 0, st, s);
  hipLaunchKernelGGL(k_minsel_resolve, res, dim3(MINSEL_THREADS), 0, st, s);
  hipLaunchKernelGGL(k_minsel_scan, dim3(s.n_chains), dim3(MINSEL_THREADS), 0, st, s.kblk, s.nb_res, s.n_kept);
}
extern "C" void mpp_launch_minsel_emit(hipStream_t st, const MinSel &s, int out_cap, int32_t *xy, double *values) {
  if (s.n_chains <= 0 || out_cap <= 0) return;
  hipLaunchKernelGGL(k_minsel_emit, dim3(s.nb_res, s.n_chains), dim3(MINSEL_THREADS), 0, st, s, out_cap, xy, values);
}
extern "C" void mpp_launch_complete_append(hipStream_t st, const MinSel &s, const DevParams *P, const TileRef *tiles, int cap, double *gain_val) {
  if (s.n_chains <= 0) return;
  hipLaunchKernelGGL(k_complete_append, dim3(s.nb_res, s.n_chains), dim3(MINSEL_THREADS), 0, st, s, P, tiles, cap, gain_val);
}
