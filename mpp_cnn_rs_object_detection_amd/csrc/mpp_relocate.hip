// mpp_relocate.hip -- relocation (mpp_move_gains, mpp_relocate): DESIGN.md section 17.  For every point v (slot i) and every
// pixel c of the window around it, u_c the map's candidate at c (birth_candidate_marks, mpp_birth.hpp), X' = X - v + u_c:
//
//   g(v, c) = E(X) - E(X') = -[ e(u_c | X') - e(v | X) + sum over the slots w != i within max_inter of v or of c, ascending,
//                               of ( e(w | X') - e(w | X) ) ]
//
//   pre-pass  one lane per point: lin, gate and e(w | X) as the birth-energy map's pre-pass caches them, and per pair term the
//             best value of the reduction, the second-best and the slot of the best.  The reductions are max / min from the
//             seed 0.0, exact selections, so red_w(X - v) is `second` when v is the slot of the best and `best` otherwise;
//   gains     one workgroup per point, one lane per window pixel.  The points within reach of the window are staged in LDS in
//             slot order, MPP_MOVE_CHUNK at a time (k_birth_map's chunking), and walked twice: the first walk completes the
//             candidate's own reductions, the second adds the neighbours' differences to e(u_c | X') - e(v | X) in slot
//             order.  Then the workgroup's arg-max on the key (-gain, row-major window index);
//   apply     one workgroup per chain: the points the selection kept (k_ptsel, mpp_descent.hip) are rewritten in place, their
//             gains go to a list in slot order;
//   round     one lane per chain books the round (relocate_book, mpp_round.hpp).
#include <cmath>

#include "mpp_birth.hpp"
#include "mpp_device.hpp"
#include "mpp_launch.hpp"
#include "mpp_round.hpp"
#include "mpp_scratch.hpp"

#define MOVE_THREADS 256
#define MOVE_WAVES (MOVE_THREADS / WAVE)
static_assert(MPP_MOVE_CHUNK >= MOVE_THREADS, "a scan of one slot per lane must fit the chunk");
static_assert((2 * MPP_MOVE_RADIUS_MAX + 1) * (2 * MPP_MOVE_RADIUS_MAX + 1) <= MOVE_THREADS, "a lane per window pixel");

extern "C" size_t mpp_move_bytes(int n_chains, int cap) {
  const size_t T = (size_t)n_chains, TC = T * cap;
  return (2 + 2 * MPP_MAX_PAIR) * TC * sizeof(double) + T * sizeof(mpp_relocate_report) + (4 + MPP_MAX_PAIR) * TC * sizeof(int32_t);
}
// (the doubles first, then the records, the ints: every array is aligned for its type)
extern "C" void mpp_move_plan(Move *m, int n_chains, int cap, void *ws) {
  const size_t T = (size_t)n_chains, TC = T * cap;
  m->n_chains = n_chains; m->cap = cap;
  double *d = (double *)ws;
  m->lin = d; m->e = d + TC; d += 2 * TC;
  for (int p = 0; p < MPP_MAX_PAIR; ++p) { m->best[p] = d; m->second[p] = d + TC; d += 2 * TC; }
  m->rep = (mpp_relocate_report *)d;
  int32_t *q = (int32_t *)(m->rep + T);
  m->gate = q; q += TC;
  for (int p = 0; p < MPP_MAX_PAIR; ++p) { m->slot[p] = q; q += TC; }
  m->to = q; q += 2 * TC;
  m->moved = q;
}

__device__ __forceinline__ int move_count(const TileRef &t, int cap) {
  const int n = *t.n;
  return n < 0 ? 0 : (n > cap ? cap : n);
}

// ---- pre-pass: one lane per point ------------------------------------------------------------------------------------------
// A reduction that remembers what it would be without its best contributor.  The seed 0.0 (slot -1) is a contributor that no
// removal takes away; equal values leave second == best.
struct Tracked { double best, second; int slot; };
__device__ __forceinline__ void track(int mode, Tracked &r, double v, int slot) {
  const bool max = mode == MPP_REDUCE_MAX;
  if (max ? v > r.best : v < r.best) { r.second = r.best; r.best = v; r.slot = slot; }
  else if (max ? v > r.second : v < r.second) r.second = v;
}

// (blockIdx.y: the chain; its grid `sstride` / `cap` entries into g, used from `grid_min` points on, as k_birth_prepass)
__global__ __launch_bounds__(WAVE) void k_move_prepass(const DevParams *P, const TileRef *tiles, Move m, Grid g, int sstride,
                                                       int grid_min, const mpp_descent_report *closed) {
  const int chain = blockIdx.y, i = blockIdx.x * WAVE + threadIdx.x;
  if (closed && closed[chain].status >= 0) return;
  TileRef t = tiles[chain];
  const int n = move_count(t, m.cap);
  if (i >= n) return;
  if (g.start && n >= grid_min) { g.start += (size_t)chain * sstride; g.items += (size_t)chain * m.cap; }
  else g = Grid{nullptr, nullptr};
  const mpp_model &M = P->model;
  const Rect u = tile_rect(t, i);
  const Geo gu = make_geo(u);
  double lin; int gate;
  unit_part<false>(P, t, &P->maps.edges[0][0], u, gu, &lin, &gate, nullptr);
  Tracked red[MPP_MAX_PAIR] = {{0.0, 0.0, -1}, {0.0, 0.0, -1}};
  const int mi = (int)ceil(P->max_inter);
  auto visit = [&](int v) {
    if (v == i) return;
    const int qx = t.px[v], qy = t.py[v];
    const int ix = u.x - qx, iy = u.y - qy;
    if (ix > mi || ix < -mi || iy > mi || iy < -mi) return;     // (the integer box first, as point_reductions)
    if (!points_interact(P, ix, iy)) return;
    const double dx = (double)ix, dy = (double)iy;
    const double d = sqrt(dx * dx + dy * dy);
    const Rect q{qx, qy, t.ps[v], t.pr[v], t.pa[v]};
    for (int p = 0; p < M.n_pair; ++p)
      if (d <= M.pair[p].max_dist) track(M.pair[p].reduce, red[p], pair_value_rects(M.pair[p], u, gu, q, d), v);
  };
  if (g.start) {                                   // (the cells point_reductions visits; the selections do not see the order)
    const int r = (int)ceil(P->max_inter / P->res);
    const int ci = grid_coord(P, u.x), cj = grid_coord(P, u.y);
    for (int a = max(ci - r, 0); a <= min(ci + r, P->nx - 1); ++a)
      for (int b = max(cj - r, 0); b <= min(cj + r, P->ny - 1); ++b) {
        const int c = b + a * P->ny;
        for (int k = g.start[c]; k < g.start[c + 1]; ++k) visit(g.items[k]);
      }
  } else {
    for (int v = 0; v < n; ++v) visit(v);
  }
  const size_t at = (size_t)chain * m.cap + i;
  m.lin[at] = lin; m.gate[at] = gate;
  for (int p = 0; p < MPP_MAX_PAIR; ++p) { m.best[p][at] = red[p].best; m.second[p][at] = red[p].second; m.slot[p][at] = red[p].slot; }
  m.e[at] = finish_energy(P, lin + pair_part(P, gate, red[0].best, red[1].best));
}

// ---- the gains: one workgroup per point, one lane per window pixel -----------------------------------------------------------
// blockDim.x: a multiple of WAVE that holds the window's (2 radius + 1)^2 pixels (mpp_launch_move_gains)
__global__ __launch_bounds__(MOVE_THREADS) void k_move_gains(const DevParams *P, const TileRef *tiles, Move m, int radius,
                                                             const mpp_descent_report *closed, double *gain) {
  // one chunk of the points within reach of the window: rectangle and cached record, in slot order
  __shared__ int32_t s_x[MPP_MOVE_CHUNK], s_y[MPP_MOVE_CHUNK], s_gate[MPP_MOVE_CHUNK], s_sl0[MPP_MOVE_CHUNK], s_sl1[MPP_MOVE_CHUNK];
  __shared__ double s_s[MPP_MOVE_CHUNK], s_r[MPP_MOVE_CHUNK], s_a[MPP_MOVE_CHUNK], s_lin[MPP_MOVE_CHUNK], s_e[MPP_MOVE_CHUNK];
  __shared__ double s_b0[MPP_MOVE_CHUNK], s_b1[MPP_MOVE_CHUNK], s_c0[MPP_MOVE_CHUNK], s_c1[MPP_MOVE_CHUNK];
  __shared__ int s_wcnt[MOVE_WAVES], s_bi[MOVE_WAVES];
  __shared__ double s_bv[MOVE_WAVES];
  const int chain = blockIdx.y, i = blockIdx.x;
  if (closed && closed[chain].status >= 0) return;               // (the whole block alike)
  TileRef t = tiles[chain];
  const int n = move_count(t, m.cap);
  if (i >= n) return;
  const mpp_model &M = P->model;
  const int H = P->H, W = P->W;
  const int nt = blockDim.x, nw = nt / WAVE, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int side = 2 * radius + 1;
  const int vx = t.px[i], vy = t.py[i];
  const int x = vx + tid / side - radius, y = vy + tid % side - radius;
  const bool live = tid < side * side && x >= 0 && x < H && y >= 0 && y < W;   // (a lane outside still scans, votes and waits)
  const double max_inter = P->max_inter;
  const int mi = (int)ceil(max_inter), reach = mi + radius;
  const size_t base = (size_t)chain * m.cap;

  // the candidate of this pixel and the part of its energy that no neighbour changes
  Rect u{live ? x : 0, live ? y : 0, 0.0, 0.0, 0.0};
  Geo gu{};
  double lin_u = 0.0;
  int gate_u = 1;
  if (live) {
    birth_candidate_marks(P, t, x, y, W, &u.s, &u.r, &u.a);
    gu = make_geo(u);
    unit_part<false>(P, t, &P->maps.edges[0][0], u, gu, &lin_u, &gate_u, nullptr);
  }
  double ru0 = 0.0, ru1 = 0.0;                // the candidate's own reductions over its neighbours in X - v
  double S = 0.0;                             // e(u_c | X') - e(v | X), then the neighbours' differences, ascending slots

  bool whole = false;                        // the first walk's one chunk held every point within reach: the second reuses it
  int cnt = 0;
  for (int pass = 0; pass < 2; ++pass) {
    int b = 0;                                // next slot to scan (the same in every lane of the block)
    bool first = true;
    do {
      if (!(pass == 1 && whole)) {
        // fill a chunk: scans of one slot per lane, each compacted by ballot in slot order, while a whole scan still fits
        cnt = 0;
        while (b < n && cnt + nt <= MPP_MOVE_CHUNK) {
          const int j = b + tid;
          int px = 0, py = 0;
          bool in = false;
          if (j < n && j != i) {
            px = t.px[j]; py = t.py[j];
            // (the points within max_inter of v or of SOME pixel of the window lie in v's box widened by ceil(max_inter) + radius)
            in = px >= vx - reach && px <= vx + reach && py >= vy - reach && py <= vy + reach;
          }
          int total;                          // (the barrier behind the stores below is the scan's second one)
          const int pos = cnt + block_scan_place_n<false>(in, nw, s_wcnt, &total);
          if (in) {                           // (pos < cnt + total <= MPP_MOVE_CHUNK)
            s_x[pos] = px; s_y[pos] = py; s_s[pos] = t.ps[j]; s_r[pos] = t.pr[j]; s_a[pos] = t.pa[j];
            s_lin[pos] = m.lin[base + j]; s_gate[pos] = m.gate[base + j]; s_e[pos] = m.e[base + j];
            s_b0[pos] = m.best[0][base + j]; s_c0[pos] = m.second[0][base + j]; s_sl0[pos] = m.slot[0][base + j];
            s_b1[pos] = m.best[1][base + j]; s_c1[pos] = m.second[1][base + j]; s_sl1[pos] = m.slot[1][base + j];
          }
          __syncthreads();                    // (the chunk is written; the wave counts may be overwritten)
          cnt += total;
          b += nt;
        }
        if (pass == 0 && first && b >= n) whole = true;
      }
      first = false;
      // walk the chunk in slot order: every lane reads the same entry (an LDS broadcast)
      if (live)
        for (int k = 0; k < cnt; ++k) {
          const int qx = s_x[k], qy = s_y[k];
          const int jx = vx - qx, jy = vy - qy;
          const bool near_v = !(jx > mi || jx < -mi || jy > mi || jy < -mi) && points_interact(P, jx, jy);
          const int ix = u.x - qx, iy = u.y - qy;
          bool near_c = !(ix > mi || ix < -mi || iy > mi || iy < -mi);
          double d = 0.0;
          if (near_c) {
            const double dx = (double)ix, dy = (double)iy;
            d = sqrt(dx * dx + dy * dy);
            near_c = d <= max_inter;
          }
          if (!near_c && (pass == 0 || !near_v)) continue;       // (the first walk is for the candidate's reductions only)
          // w's reductions without v: the second-best where v is the slot of the best
          double nv0 = s_sl0[k] == i ? s_c0[k] : s_b0[k], nv1 = s_sl1[k] == i ? s_c1[k] : s_b1[k];
          if (near_c) {
            const Rect q{qx, qy, s_s[k], s_r[k], s_a[k]};
            // pair(w, u_c) = pair(u_c, w) bit for bit (mpp_scratch.hpp): one evaluation serves both points' reductions
            if (M.n_pair > 0 && d <= M.pair[0].max_dist) {
              const double v = pair_value_rects(M.pair[0], u, gu, q, d);
              ru0 = pass == 0 ? reduce2(M.pair[0].reduce, ru0, v) : ru0; nv0 = reduce2(M.pair[0].reduce, nv0, v);
            }
            if (M.n_pair > 1 && d <= M.pair[1].max_dist) {
              const double v = pair_value_rects(M.pair[1], u, gu, q, d);
              ru1 = pass == 0 ? reduce2(M.pair[1].reduce, ru1, v) : ru1; nv1 = reduce2(M.pair[1].reduce, nv1, v);
            }
          }
          if (pass == 1) S += finish_energy(P, s_lin[k] + pair_part(P, s_gate[k], nv0, nv1)) - s_e[k];
        }
      __syncthreads();                        // (every lane is done with the chunk before the next one is staged)
    } while (b < n && !(pass == 1 && whole));
    if (pass == 0) S = finish_energy(P, lin_u + pair_part(P, gate_u, ru0, ru1)) - m.e[base + i];
  }

  // the workgroup's arg-max on (-gain, window index): the largest non-NaN g, ties to the smaller row, then the smaller column
  double bv = -S;
  int bi = (live && bv == bv) ? tid : -1;     // (-1: no value)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v2 = __shfl_xor(bv, o, WAVE);
    const int i2 = __shfl_xor(bi, o, WAVE);
    if (i2 >= 0 && (bi < 0 || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
  }
  if (lane == 0) { s_bv[wave] = bv; s_bi[wave] = bi; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < nw; ++w) {
    const double v2 = s_bv[w];
    const int i2 = s_bi[w];
    if (i2 >= 0 && (bi < 0 || v2 > bv || (v2 == bv && i2 < bi))) { bv = v2; bi = i2; }
  }
  gain[base + i] = bi >= 0 ? bv : __longlong_as_double(0x7ff8000000000000ll);
  m.to[2 * (base + i)] = bi >= 0 ? vx + bi / side - radius : -1;
  m.to[2 * (base + i) + 1] = bi >= 0 ? vy + bi % side - radius : -1;
}

// ---- the round ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void k_move_init(const TileRef *tiles, Move m) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.n_chains) return;
  mpp_relocate_report r{};                                       // (the counts and the gain start at 0)
  r.status = -1; r.n_after = move_count(tiles[c], m.cap); r.slot_max = -1; r.max_gain = -HUGE_VAL;
  m.rep[c] = r;
}

// The points the selection kept in an open chain are rewritten in place: position to[i], the marks of the map's candidate
// there.  rem_val[chain][place]: the kept gains in slot order; n_rem[chain]: their number.
__global__ __launch_bounds__(MOVE_THREADS) void k_move_apply(const DevParams *P, const TileRef *tiles, Move m, Descent d) {
  __shared__ int s_tot[MOVE_WAVES];
  const int chain = blockIdx.x, tid = threadIdx.x;
  if (d.rep[chain].status >= 0) return;                          // (closed: not touched again)
  TileRef t = tiles[chain];
  const int n = move_count(t, m.cap);
  const size_t o = (size_t)chain * m.cap;
  int n_kept = 0;
  for (int base = 0; base < n; base += MOVE_THREADS) {
    const int i = base + tid;
    int x = -1, y = -1;
    if (i < n && d.keep[o + i] != 0) { x = m.to[2 * (o + i)]; y = m.to[2 * (o + i) + 1]; }
    const bool kept = x >= 0 && x < P->H && y >= 0 && y < P->W;   // (a kept point has a gain, so a pixel of the tile)
    int total;
    const int place = n_kept + block_scan_place<MOVE_WAVES>(kept, s_tot, &total);
    if (kept) {
      double s, r, a;
      birth_candidate_marks(P, t, x, y, P->W, &s, &r, &a);
      t.px[i] = x; t.py[i] = y; t.ps[i] = s; t.pr[i] = r; t.pa[i] = a;
      d.rem_val[o + place] = d.p[o + i];                         // (place <= i < cap)
      m.moved[o + i] += 1;
    }
    n_kept += total;
  }
  if (tid == 0) d.n_rem[chain] = n_kept;
}

// one lane per chain: the round's book
__global__ __launch_bounds__(WAVE) void k_move_round(const TileRef *tiles, Move m, Descent d, int max_rounds) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.n_chains || d.rep[c].status >= 0) return;
  mpp_relocate_report r = m.rep[c];
  relocate_book(r, max_rounds, tiles[c].err, d.n_rem[c], d.rem_val + (size_t)c * m.cap);
  m.rep[c] = r;
  d.rep[c].status = r.status;                                    // (what the selection and the next round's kernels read)
}

// the summary of the returned state's gains (k_descent_summary's max_p, slot_max, n_positive) goes into the books
__global__ __launch_bounds__(WAVE) void k_move_finish(Move m, Descent d) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m.n_chains) return;
  m.rep[c].max_gain = d.rep[c].max_p; m.rep[c].slot_max = d.rep[c].slot_max; m.rep[c].n_positive = (int32_t)d.rep[c].n_positive;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
extern "C" void mpp_launch_move_gains(hipStream_t st, const DevParams *P, const TileRef *tiles, const Move &m, const Descent &d,
                                      int radius, const int32_t *grid_start, const int32_t *grid_items, int sstride, int grid_min,
                                      int skip_closed) {
  if (m.n_chains <= 0 || m.cap <= 0) return;
  const mpp_descent_report *closed = skip_closed ? d.rep : nullptr;
  hipLaunchKernelGGL(k_move_prepass, dim3((m.cap + WAVE - 1) / WAVE, m.n_chains), dim3(WAVE), 0, st, P, tiles, m,
                     Grid{grid_start, grid_items}, sstride, grid_min, closed);
  const int side = 2 * radius + 1, threads = (side * side + WAVE - 1) / WAVE * WAVE;
  hipLaunchKernelGGL(k_move_gains, dim3(m.cap, m.n_chains), dim3(threads), 0, st, P, tiles, m, radius, closed, d.p);
}
extern "C" void mpp_launch_move_init(hipStream_t st, const TileRef *tiles, const Move &m) {
  if (m.n_chains <= 0) return;
  hipLaunchKernelGGL(k_move_init, dim3((m.n_chains + WAVE - 1) / WAVE), dim3(WAVE), 0, st, tiles, m);
}
extern "C" void mpp_launch_move_apply(hipStream_t st, const DevParams *P, const TileRef *tiles, const Move &m, const Descent &d) {
  if (m.n_chains <= 0) return;
  hipLaunchKernelGGL(k_move_apply, dim3(m.n_chains), dim3(MOVE_THREADS), 0, st, P, tiles, m, d);
}
extern "C" void mpp_launch_move_round(hipStream_t st, const TileRef *tiles, const Move &m, const Descent &d, int max_rounds) {
  if (m.n_chains <= 0) return;
  hipLaunchKernelGGL(k_move_round, dim3((m.n_chains + WAVE - 1) / WAVE), dim3(WAVE), 0, st, tiles, m, d, max_rounds);
}
extern "C" void mpp_launch_move_finish(hipStream_t st, const Move &m, const Descent &d) {
  if (m.n_chains <= 0) return;
  hipLaunchKernelGGL(k_move_finish, dim3((m.n_chains + WAVE - 1) / WAVE), dim3(WAVE), 0, st, m, d);
}
