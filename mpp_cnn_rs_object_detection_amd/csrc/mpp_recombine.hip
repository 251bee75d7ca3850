// mpp_recombine.hip -- recombination of restarts: per tile, the best replica per interaction cluster (the
// rules are stated in include/mpp_hip.h at mpp_recombine).
//
// One workgroup per tile.  The points of the tile's R replicas are taken in the compact order k = off[r] + slot (replica after
// replica, slots ascending), which is the order of the global index g = r * cap + slot: the smallest k of a cluster is its
// smallest g.  The stages, each over the whole workgroup, a barrier between two:
//   winner and offsets     one lane: the rule of select_replicas over the R chain energies, the prefix of the R counts
//   labels                 lab[k] = k, then sweeps: every point takes the smallest label among itself and the points it is
//                          linked to (a scan over the tile's points: integer box test, then points_interact), follows that
//                          label's own label down to a root, and stores the result.  A label only ever decreases and never
//                          below its cluster's smallest index, and a sweep that changes nothing has read nothing but final
//                          values, so the fixed point -- every member holds its cluster's smallest index -- does not depend
//                          on which of two racing lanes came first.  No fixed sweep count.
//   choice                 one lane per cluster root: S[r] over the root's members, replica by replica in slot order (rules 5, 6)
//   E_sum, counts          a ballot scan compacts the roots in ascending order; one lane adds their chosen sums in that order
//   composite              replicas in walk order, a workgroup of slots at a time; a ballot scan places the kept points in the staging rows
//   write                  status 1 only: staging rows -> the winner chain
// Labels, packed positions, choices and chosen sums live in LDS while the tile has at most lds_points points, else in the
// call's workspace: the stages are one function, inlined once for each of the two address spaces (rc_tile).
#include "mpp_device.hpp"
#include "mpp_launch.hpp"
#include "mpp_scratch.hpp"      // points_interact

#define RC_THREADS 1024
#define RC_WAVES (RC_THREADS / WAVE)

// The stages of one tile after the winner and the offsets are known.  Inlined twice, with the four arrays in LDS and in the
// workspace: each copy addresses them in their own address space (one body behind pointers chosen at run time would read the
// LDS through flat loads).  sh: {changed, taken} and the scan's wave totals, in LDS.
__device__ __forceinline__ void rc_tile(const DevParams *P, const TileRef *tiles, const Recomb &rc, const double *e_pts,
                                        const int32_t *off, mpp_recombine_report *rep, const int w, const int N, int32_t *lab,
                                        int32_t *choice, uint32_t *xy, double *chosen, int *sh, int *s_wave) {
  const int i = blockIdx.x, tid = threadIdx.x, n = rc.n, R = rc.R, cap = rc.cap;
  for (int r = 0; r < R; ++r) {
    const TileRef &t = tiles[r * n + i];
    const int o = off[r], nr = off[r + 1] - o;
    for (int s = tid; s < nr; s += RC_THREADS) {
      xy[o + s] = ((uint32_t)t.px[s] << 16) | ((uint32_t)t.py[s] & 0xffffu);
      lab[o + s] = o + s;
    }
  }

  // ---- labels.  Within a sweep other lanes of the workgroup write labels this lane reads: the accesses are relaxed atomics
  // of workgroup scope, so every read takes a value some lane stored (any of them will do, see the file header) and none is
  // kept in a register across the scan; between two sweeps stands a barrier.
  auto label = [&](int k) { return __hip_atomic_load(&lab[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
  const int mi = (int)ceil(P->max_inter);
  for (;;) {
    __syncthreads();
    if (tid == 0) sh[0] = 0;
    __syncthreads();
    bool changed = false;
    for (int k = tid; k < N; k += RC_THREADS) {
      const uint32_t pk = xy[k];
      const int xk = (int)(pk >> 16), yk = (int)(pk & 0xffffu), m0 = label(k);
      int m = m0;
      auto visit = [&](int j, uint32_t pj) {                      // (integer box test first: almost every point fails it)
        const int ix = xk - (int)(pj >> 16), iy = yk - (int)(pj & 0xffffu);
        if (ix <= mi && ix >= -mi && iy <= mi && iy >= -mi && points_interact(P, ix, iy)) m = min(m, label(j));
      };
      int j = 0;
      for (; j + 4 <= N; j += 4) {                                // (four independent loads per turn: their latencies overlap)
        const uint32_t p0 = xy[j], p1 = xy[j + 1], p2 = xy[j + 2], p3 = xy[j + 3];
        visit(j, p0); visit(j + 1, p1); visit(j + 2, p2); visit(j + 3, p3);
      }
      for (; j < N; ++j) visit(j, xy[j]);
      for (int up = label(m); up < m; up = label(m)) m = up;      // pointer jumping: lab[m] <= m, a root has lab[m] == m
      if (m < m0) { __hip_atomic_store(&lab[k], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); changed = true; }
    }
    if (changed) sh[0] = 1;
    __syncthreads();
    if (!sh[0]) break;
  }

  // ---- the choice of every cluster (its root: lab[k] == k)
  for (int k = tid; k < N; k += RC_THREADS) {
    if (lab[k] != k) continue;
    int best = w;
    double sb = 0.0;
    for (int q = -1; q < R; ++q) {                                 // the winner first, then 0 .. R-1 without it
      const int r = q < 0 ? w : q;
      if (q == w) continue;
      const double *e = e_pts + (size_t)(r * n + i) * cap;
      const int o = off[r], hi = off[r + 1];
      double s = 0.0;
      for (int p = max(o, k); p < hi; ++p)                         // (no member of the cluster lies before its root)
        if (lab[p] == k) s += e[p - o];
      if (q < 0) sb = s;
      else if (s < sb || (!isfinite(sb) && isfinite(s))) { best = r; sb = s; }
    }
    choice[k] = best; chosen[k] = sb;
  }
  __syncthreads();

  // ---- the roots, compacted in ascending order (into xy: the positions have done their work), then one lane adds the chosen
  // sums in that order -- the only part of E_sum that has to be serial
  int ncl = 0;
  for (int k0 = 0; k0 < N; k0 += RC_THREADS) {
    const int k = k0 + tid;
    const bool root = k < N && lab[k] == k;
    int total;
    const int pos = ncl + block_scan_place<RC_WAVES>(root, s_wave, &total);
    if (root) xy[pos] = (uint32_t)k;
    ncl += total;
  }
  __syncthreads();
  if (tid == 0) {
    int taken = 0;
    double es = 0.0;
    for (int q = 0; q < ncl; ++q) {
      const int k = (int)xy[q];
      taken += choice[k] != w ? 1 : 0; es += chosen[k];
    }
    rep->n_clusters = ncl; rep->n_taken = taken; rep->E_sum = es;
    sh[1] = taken;
  }
  __syncthreads();
  const int taken = sh[1], nw = off[w + 1] - off[w];

  // ---- the composite, staged
  const size_t row = (size_t)i * cap;
  int32_t *src = rc.src + 2 * row;
  int m = nw;
  if (taken > 0) {
    m = 0;
    for (int q = -1; q < R; ++q) {
      const int r = q < 0 ? w : q;
      if (q == w) continue;
      const TileRef &t = tiles[r * n + i];
      const int o = off[r], nr = off[r + 1] - o;
      for (int s0 = 0; s0 < nr; s0 += RC_THREADS) {
        const int s = s0 + tid;
        const bool keep = s < nr && choice[lab[o + s]] == r;
        int total;
        const int pos = m + block_scan_place<RC_WAVES>(keep, s_wave, &total);
        if (keep && pos < cap) {
          rc.spx[row + pos] = t.px[s]; rc.spy[row + pos] = t.py[s];
          rc.sps[row + pos] = t.ps[s]; rc.spr[row + pos] = t.pr[s]; rc.spa[row + pos] = t.pa[s];
          src[2 * pos] = r; src[2 * pos + 1] = s;
        }
        m += total;
      }
    }
  }
  const int status = taken == 0 ? 0 : (m > cap ? 2 : 1);
  __syncthreads();                                                 // every source row is read, every staged row written
  const int n_after = status == 1 ? m : nw;
  if (status == 1) {
    const TileRef &d = tiles[w * n + i];
    for (int k = tid; k < m; k += RC_THREADS) {
      d.px[k] = rc.spx[row + k]; d.py[k] = rc.spy[row + k];
      d.ps[k] = rc.sps[row + k]; d.pr[k] = rc.spr[row + k]; d.pa[k] = rc.spa[row + k];
    }
    if (tid == 0) { *d.n = m; *d.err = 0; }
  } else {
    for (int k = tid; k < nw; k += RC_THREADS) { src[2 * k] = w; src[2 * k + 1] = k; }
  }
  for (int k = n_after + tid; k < cap; k += RC_THREADS) { src[2 * k] = -1; src[2 * k + 1] = -1; }
  if (tid == 0) { rep->status = status; rep->n_after = n_after; }
}

__global__ __launch_bounds__(RC_THREADS) void k_recombine(const DevParams *P, const TileRef *tiles, Recomb rc, const double *e_pts,
                                                          const double *e_sum, int lds_points) {
  __shared__ int32_t s_lab[MPP_RECOMBINE_LDS_POINTS], s_choice[MPP_RECOMBINE_LDS_POINTS];
  __shared__ __attribute__((aligned(16))) uint32_t s_xy[MPP_RECOMBINE_LDS_POINTS];
  __shared__ double s_chosen[MPP_RECOMBINE_LDS_POINTS];
  __shared__ int s_w, s_N, s_flags[2], s_wave[RC_WAVES];
  const int i = blockIdx.x, tid = threadIdx.x, n = rc.n, R = rc.R, cap = rc.cap;
  int32_t *off = rc.off + (size_t)i * (R + 1);
  mpp_recombine_report *rep = rc.rep + i;

  if (tid == 0) {
    int w = 0, tot = 0;
    double be = e_sum[i];
    off[0] = 0;
    for (int r = 0; r < R; ++r) {
      const int c = r * n + i;
      tot += min(*tiles[c].n, cap);
      off[r + 1] = tot;
      const double e = e_sum[c];
      if (r > 0 && (e < be || (!isfinite(be) && isfinite(e)))) { w = r; be = e; }
    }
    s_w = w; s_N = tot;
    rep->winner = w; rep->E_winner = be; rep->E_after = be;
    rep->n_before = off[w + 1] - off[w];
  }
  __syncthreads();
  const int w = s_w, N = s_N;
  const bool lds = N <= lds_points && N <= MPP_RECOMBINE_LDS_POINTS;
  const size_t big = (size_t)i * R * cap;
  if (lds) rc_tile(P, tiles, rc, e_pts, off, rep, w, N, s_lab, s_choice, s_xy, s_chosen, s_flags, s_wave);
  else rc_tile(P, tiles, rc, e_pts, off, rep, w, N, rc.lab + big, rc.choice + big, rc.xy + big, rc.chosen + big, s_flags, s_wave);
}

// E_after: the winner chain's energy in the written state (for status 0 and 2 the chain is as it was: the same bits)
__global__ void k_recombine_after(Recomb rc, const double *e_sum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rc.n) rc.rep[i].E_after = e_sum[rc.rep[i].winner * rc.n + i];
}

static size_t rc_align(size_t b) { return (b + 15) & ~(size_t)15; }
extern "C" size_t mpp_recombine_bytes(int n, int R, int cap) {
  const size_t big = (size_t)n * R * cap, row = (size_t)n * cap;
  return rc_align(big * sizeof(double)) + 3 * rc_align(row * sizeof(double)) + rc_align((size_t)n * sizeof(mpp_recombine_report)) +
         3 * rc_align(big * sizeof(int32_t)) + 2 * rc_align(row * sizeof(int32_t)) + rc_align(2 * row * sizeof(int32_t)) +
         rc_align((size_t)n * (R + 1) * sizeof(int32_t));
}
extern "C" void mpp_recombine_plan(Recomb *rc, int n, int R, int cap, void *ws) {
  const size_t big = (size_t)n * R * cap, row = (size_t)n * cap;
  unsigned char *p = (unsigned char *)ws;
  auto take = [&](size_t bytes) { void *q = p; p += rc_align(bytes); return q; };
  rc->n = n; rc->R = R; rc->cap = cap;
  rc->chosen = (double *)take(big * sizeof(double));
  rc->sps = (double *)take(row * sizeof(double)); rc->spr = (double *)take(row * sizeof(double)); rc->spa = (double *)take(row * sizeof(double));
  rc->rep = (mpp_recombine_report *)take((size_t)n * sizeof(mpp_recombine_report));
  rc->lab = (int32_t *)take(big * sizeof(int32_t)); rc->choice = (int32_t *)take(big * sizeof(int32_t));
  rc->xy = (uint32_t *)take(big * sizeof(uint32_t));
  rc->spx = (int32_t *)take(row * sizeof(int32_t)); rc->spy = (int32_t *)take(row * sizeof(int32_t));
  rc->src = (int32_t *)take(2 * row * sizeof(int32_t));
  rc->off = (int32_t *)take((size_t)n * (R + 1) * sizeof(int32_t));
}
extern "C" void mpp_launch_recombine(hipStream_t st, const DevParams *P, const TileRef *tiles, const Recomb &rc, const double *e_pts,
                                     const double *e_sum, int lds_points) {
  if (rc.n <= 0) return;
  hipLaunchKernelGGL(k_recombine, dim3(rc.n), dim3(RC_THREADS), 0, st, P, tiles, rc, e_pts, e_sum, lds_points);
}
extern "C" void mpp_launch_recombine_after(hipStream_t st, const Recomb &rc, const double *e_sum) {
  if (rc.n <= 0) return;
  hipLaunchKernelGGL(k_recombine_after, dim3((rc.n + WAVE - 1) / WAVE), dim3(WAVE), 0, st, rc, e_sum);
}
