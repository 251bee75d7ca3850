// mpp_birth_map.hip -- the birth-energy map: dE(c) = E(X + u_c) - E(X) for EVERY pixel c of every chain, u_c the rectangle
// ShapeNet proposes at c (the argmax class of each mark map, at its lower bin edge).  exp(-dE) is the conditional
// (Papangelou) intensity of the point process where there is no detection (the reference's utils/figures/ show_papangelou);
// dE(c) < 0 anywhere means the configuration is not a local minimum with respect to births.  DESIGN.md section 12.
//
//   dE(c) = e(u_c | X + u_c) + sum over the slots v with d(v, c) <= max_inter, ascending, of [ e(v | X + u_c) - e(v | X) ]
//
// The pair reductions are max / min over the neighbours, so red_v(X + u_c) = reduce2(red_v(X), pair(v, u_c)) is the
// from-scratch reduction bit for bit.  A pre-pass caches per point what does not depend on c -- lin, gate, the reductions and
// e(v | X), through point_reductions of mpp_scratch.hpp, the code of mpp_total_energy -- and the map kernel, one lane per
// pixel, adds the candidate to the cached reductions of the points near its block of pixels, staged in LDS.
#include "mpp_birth.hpp"
#include "mpp_device.hpp"
#include "mpp_launch.hpp"
#include "mpp_scratch.hpp"

// ---- pre-pass: one lane per point --------------------------------------------------------------------------------------
// (blockIdx.y: the chain; its grid `sstride` / `cap` entries into g, used from `grid_min` points on, as k_point_energies)
__global__ __launch_bounds__(64) void k_birth_prepass(const DevParams *P, const TileRef *tiles, int cap, BirthCache bc, Grid g,
                                                      int sstride, int grid_min) {
  const int chain = blockIdx.y, i = blockIdx.x * WAVE + threadIdx.x;
  TileRef t = tiles[chain];
  const int n = min(*t.n, cap);
  if (i >= n) return;
  if (g.start && n >= grid_min) { g.start += (size_t)chain * sstride; g.items += (size_t)chain * cap; }
  else g = Grid{nullptr, nullptr};
  const Overlay none{0, nullptr, 0, nullptr, nullptr};
  const Rect u = tile_rect(t, i);
  const Geo gu = make_geo(u);
  double lin; int gate;
  unit_part<false>(P, t, &P->maps.edges[0][0], u, gu, &lin, &gate, nullptr);
  double red[MPP_MAX_PAIR] = {0.0, 0.0};
  point_reductions(P, t, n, u, gu, i, -1, none, g, red);
  const size_t at = (size_t)chain * cap + i;
  bc.lin[at] = lin; bc.gate[at] = gate; bc.r0[at] = red[0]; bc.r1[at] = red[1];
  bc.e[at] = finish_energy(P, lin + pair_part(P, gate, red[0], red[1]));
}

// ---- the map: one workgroup per BX x BY pixels, one lane per pixel ---------------------------------------------------------
#define BIRTH_BX 8          // rows of a block
#define BIRTH_BY 32         // columns of a block: a wave covers two rows of 32 pixels
#define BIRTH_THREADS (BIRTH_BX * BIRTH_BY)
static_assert(MPP_BIRTH_CHUNK >= BIRTH_THREADS, "a scan of one slot per lane must fit the chunk");

__global__ __launch_bounds__(BIRTH_THREADS) void k_birth_map(const DevParams *P, const TileRef *tiles, int cap, BirthCache bc,
                                                             double *dE, double *marks) {
  // one chunk of the points within reach of the block: rectangle and cached record, in slot order
  __shared__ int32_t s_x[MPP_BIRTH_CHUNK], s_y[MPP_BIRTH_CHUNK], s_gate[MPP_BIRTH_CHUNK];
  __shared__ double s_s[MPP_BIRTH_CHUNK], s_r[MPP_BIRTH_CHUNK], s_a[MPP_BIRTH_CHUNK];
  __shared__ double s_lin[MPP_BIRTH_CHUNK], s_r0[MPP_BIRTH_CHUNK], s_r1[MPP_BIRTH_CHUNK], s_e[MPP_BIRTH_CHUNK];
  __shared__ int s_wcnt[BIRTH_THREADS / WAVE];
  const mpp_model &M = P->model;
  const int chain = blockIdx.z, H = P->H, W = P->W;
  TileRef t = tiles[chain];
  const int n = min(*t.n, cap);
  const int tid = threadIdx.y * BIRTH_BY + threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int x0 = blockIdx.y * BIRTH_BX, y0 = blockIdx.x * BIRTH_BY;
  const int x = x0 + threadIdx.y, y = y0 + threadIdx.x;
  const bool live = x < H && y < W;           // (a lane outside the tile still scans, votes and waits with its block)
  const double max_inter = P->max_inter;
  const int mi = (int)ceil(max_inter);

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
  double ru0 = 0.0, ru1 = 0.0;                // the candidate's own reductions over its neighbours
  double acc = 0.0;                           // sum of e(v | X + u_c) - e(v | X), ascending slots

  const unsigned long long below = (1ull << lane) - 1ull;
  const size_t base = (size_t)chain * cap;
  int b = 0;                                  // next slot to scan (the same in every lane of the block)
  while (b < n) {
    // fill a chunk: scans of one slot per lane, each compacted by ballot in slot order, while a whole scan still fits
    int cnt = 0;
    while (b < n && cnt + BIRTH_THREADS <= MPP_BIRTH_CHUNK) {
      const int i = b + tid;
      int px = 0, py = 0;
      bool in = false;
      if (i < n) {
        px = t.px[i]; py = t.py[i];
        // (the points within max_inter of SOME pixel of the block lie in the block's box widened by ceil(max_inter))
        in = px >= x0 - mi && px <= x0 + BIRTH_BX - 1 + mi && py >= y0 - mi && py <= y0 + BIRTH_BY - 1 + mi;
      }
      const unsigned long long m = __ballot(in);
      if (lane == 0) s_wcnt[wave] = __popcll(m);
      __syncthreads();
      int pos = cnt + __popcll(m & below), total = 0;
#pragma unroll
      for (int w = 0; w < BIRTH_THREADS / WAVE; ++w) {
        const int c = s_wcnt[w];
        pos += w < wave ? c : 0;
        total += c;
      }
      if (in) {                               // (pos < cnt + total <= MPP_BIRTH_CHUNK)
        s_x[pos] = px; s_y[pos] = py; s_s[pos] = t.ps[i]; s_r[pos] = t.pr[i]; s_a[pos] = t.pa[i];
        s_lin[pos] = bc.lin[base + i]; s_gate[pos] = bc.gate[base + i];
        s_r0[pos] = bc.r0[base + i]; s_r1[pos] = bc.r1[base + i]; s_e[pos] = bc.e[base + i];
      }
      __syncthreads();                        // (the chunk is written; the wave counts may be overwritten)
      cnt += total;
      b += BIRTH_THREADS;
    }
    // walk the chunk in slot order: every lane reads the same entry (an LDS broadcast)
    if (live)
      for (int k = 0; k < cnt; ++k) {
        const int ix = u.x - s_x[k], iy = u.y - s_y[k];
        if (ix > mi || ix < -mi || iy > mi || iy < -mi) continue;
        const double dx = (double)ix, dy = (double)iy;
        const double d = sqrt(dx * dx + dy * dy);
        if (d > max_inter) continue;
        const Rect q{s_x[k], s_y[k], s_s[k], s_r[k], s_a[k]};
        // pair(v, u_c) = pair(u_c, v) bit for bit (mpp_scratch.hpp): one evaluation serves both points' reductions
        double nv0 = s_r0[k], nv1 = s_r1[k];
        if (M.n_pair > 0 && d <= M.pair[0].max_dist) {
          const double v = pair_value_rects(M.pair[0], u, gu, q, d);
          ru0 = reduce2(M.pair[0].reduce, ru0, v); nv0 = reduce2(M.pair[0].reduce, nv0, v);
        }
        if (M.n_pair > 1 && d <= M.pair[1].max_dist) {
          const double v = pair_value_rects(M.pair[1], u, gu, q, d);
          ru1 = reduce2(M.pair[1].reduce, ru1, v); nv1 = reduce2(M.pair[1].reduce, nv1, v);
        }
        acc += finish_energy(P, s_lin[k] + pair_part(P, s_gate[k], nv0, nv1)) - s_e[k];
      }
    __syncthreads();                          // (every lane is done with the chunk before the next one is staged)
  }
  if (!live) return;
  const size_t o = ((size_t)chain * H + x) * W + y;
  dE[o] = acc + finish_energy(P, lin_u + pair_part(P, gate_u, ru0, ru1));
  if (marks) { marks[3 * o] = u.s; marks[3 * o + 1] = u.r; marks[3 * o + 2] = u.a; }
}

// ---- the summary: smallest non-NaN value (ties: smallest index), pixels below 0, NaN pixels -----------------------------------
__device__ __forceinline__ void birth_merge(BirthPart &a, const BirthPart &b) {
  if (b.idx >= 0 && (a.idx < 0 || b.v < a.v || (b.v == a.v && b.idx < a.idx))) { a.v = b.v; a.idx = b.idx; }
  a.n_neg += b.n_neg; a.n_nan += b.n_nan;
}
__device__ __forceinline__ BirthPart birth_block_reduce(BirthPart p, BirthPart *sh) {
  sh[threadIdx.x] = p;
  __syncthreads();
  for (int s = (int)blockDim.x / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) birth_merge(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  return sh[0];
}
// (the counts are integers and the minimum is order-free: the partition into parts does not show in the result)
__global__ __launch_bounds__(256) void k_birth_summary_parts(long long hw, const double *dE, BirthPart *part) {
  __shared__ BirthPart sh[256];
  const double *d = dE + (size_t)blockIdx.y * hw;
  BirthPart p{INFINITY, -1, 0, 0};
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < hw; i += 256ll * gridDim.x) {
    const double v = d[i];
    if (v != v) { ++p.n_nan; continue; }
    if (v < 0.0) ++p.n_neg;
    if (p.idx < 0 || v < p.v) { p.v = v; p.idx = i; }      // (ascending i: the first of equal values stays)
  }
  p = birth_block_reduce(p, sh);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * MPP_BIRTH_PARTS + blockIdx.x] = p;
}
__global__ __launch_bounds__(MPP_BIRTH_PARTS) void k_birth_summary_final(int n_parts, int W, const BirthPart *part,
                                                                         mpp_birth_summary *out) {
  __shared__ BirthPart sh[MPP_BIRTH_PARTS];
  BirthPart p{INFINITY, -1, 0, 0};
  if ((int)threadIdx.x < n_parts) p = part[(size_t)blockIdx.x * MPP_BIRTH_PARTS + threadIdx.x];
  p = birth_block_reduce(p, sh);
  if (threadIdx.x == 0) {
    mpp_birth_summary s;
    s.min_dE = p.idx >= 0 ? p.v : (double)INFINITY;
    s.x = p.idx >= 0 ? (int32_t)(p.idx / W) : -1;
    s.y = p.idx >= 0 ? (int32_t)(p.idx % W) : -1;
    s.n_negative = p.n_neg; s.n_nan = p.n_nan;
    out[blockIdx.x] = s;
  }
}

extern "C" void mpp_launch_birth_prepass(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_chains, int cap,
                                         BirthCache bc, const int32_t *grid_start, const int32_t *grid_items, int sstride,
                                         int grid_min) {
  if (n_chains <= 0 || cap <= 0) return;
  hipLaunchKernelGGL(k_birth_prepass, dim3((cap + WAVE - 1) / WAVE, n_chains), dim3(WAVE), 0, st, P, tiles, cap, bc,
                     Grid{grid_start, grid_items}, sstride, grid_min);
}
extern "C" void mpp_launch_birth_map(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_chains, int cap, int H, int W,
                                     BirthCache bc, double *dE, double *marks) {
  if (n_chains <= 0 || H <= 0 || W <= 0) return;
  hipLaunchKernelGGL(k_birth_map, dim3((W + BIRTH_BY - 1) / BIRTH_BY, (H + BIRTH_BX - 1) / BIRTH_BX, n_chains),
                     dim3(BIRTH_BY, BIRTH_BX), 0, st, P, tiles, cap, bc, dE, marks);
}
extern "C" void mpp_launch_birth_summary(hipStream_t st, int n_chains, int H, int W, const double *dE, BirthPart *part,
                                         mpp_birth_summary *out) {
  if (n_chains <= 0) return;
  const long long hw = (long long)H * W;
  const int n_parts = (int)((hw + 255) / 256 < MPP_BIRTH_PARTS ? (hw + 255) / 256 : MPP_BIRTH_PARTS);
  hipLaunchKernelGGL(k_birth_summary_parts, dim3(n_parts, n_chains), dim3(256), 0, st, hw, dE, part);
  hipLaunchKernelGGL(k_birth_summary_final, dim3(n_chains), dim3(MPP_BIRTH_PARTS), 0, st, n_parts, W, (const BirthPart *)part, out);
}
