// mpp_scratch.hpp -- the from-scratch energy of one point, shared by the kernels that evaluate it on the configuration in
// HBM (mpp_scratch.hip: total energy, deltas, Papangelou; mpp_birth_map.hip: the per-point cache of the birth-energy map).
// One definition, so that every caller gets the same bits (the library is built with -ffp-contract=off).
#pragma once
#include "mpp_device.hpp"

struct Grid {                 // CSR over the P->nx x P->ny cells of the tile: items[start[c] .. start[c+1]) = slots in cell c
  const int32_t *start;       // nullptr: no grid, scan all points
  const int32_t *items;
};
__device__ __forceinline__ int grid_coord(const DevParams *P, int x) {
  return P->res_shift >= 0 ? (x >> P->res_shift) : (x / P->res_int);
}

// "u and v interact": the centres, (ix, iy) apart, lie within the model's largest pair range.  The one statement of the
// predicate the from-scratch kernels evaluate inline (point_reductions below, the touched / listed tests of mpp_scratch.hip and
// mpp_birth_map.hip keep their own copies of the expression: it is the same arithmetic, and their code is not touched).
// What links two points of mpp_recombine (mpp_recombine.hip).
__device__ __forceinline__ bool points_interact(const DevParams *P, int ix, int iy) {
  const double dx = (double)ix, dy = (double)iy;
  return sqrt(dx * dx + dy * dy) <= P->max_inter;
}

struct Overlay {
  int n_excl; const int32_t *excl;          // slots removed
  int n_extra; const int32_t *exy; const double *emarks;   // rectangles added
};

__device__ __forceinline__ Rect tile_rect(const TileRef &t, int i) {
  return Rect{t.px[i], t.py[i], t.ps[i], t.pr[i], t.pa[i]};
}
__device__ __forceinline__ Rect extra_rect(const Overlay &o, int e) {
  return Rect{o.exy[2 * e], o.exy[2 * e + 1], o.emarks[3 * e], o.emarks[3 * e + 1], o.emarks[3 * e + 2]};
}
__device__ __forceinline__ bool excluded(const Overlay &o, int slot) {
  for (int i = 0; i < o.n_excl; ++i) if (o.excl[i] == slot) return true;
  return false;
}
// (a function of the unordered pair, bit for bit: the overlap clips the smaller rectangle -- rect_less -- against the larger,
// min, the sum of the radii and the squared distance are symmetric, and the alignment's products commute)
__device__ inline double pair_value_rects(const mpp_pair_term &pt, const Rect &u, const Geo &gu, const Rect &v, double d) {
  switch (pt.kind) {
    case MPP_P_OVERLAP: {
      Geo gv = make_geo(v);
      bool uf = rect_less(u.x, u.y, u.s, u.r, u.a, v.x, v.y, v.s, v.r, v.a);
      return overlap_energy(gu, gv, uf);
    }
    case MPP_P_ALIGN: {
      Geo gv = make_geo(v);
      return 1.0 - fabs(gu.ca * gv.ca + gu.sa * gv.sa) - (pt.p[0] != 0.0 ? 1.0 : 0.0);
    }
    case MPP_P_DIST_LE: return d <= pt.max_dist ? 1.0 : 0.0;
    case MPP_P_DIST_LT: return d < pt.max_dist ? 1.0 : 0.0;
  }
  return 0.0;
}

// the pair reductions red[0 .. n_pair) (from 0.0) of rectangle u in the state (configuration - excluded + extras)
__device__ inline void point_reductions(const DevParams *P, const TileRef &t, int n, const Rect &u, const Geo &gu, int self_slot,
                                        int self_extra, const Overlay &o, const Grid &g, double *red) {
  const mpp_model &M = P->model;
  const int mi = (int)ceil(P->max_inter);
  auto visit = [&](int v) {                       // v < n: slot of the configuration, else added rectangle v - n
    Rect q;
    if (v < n) {
      if (v == self_slot || excluded(o, v)) return;
      q.x = t.px[v]; q.y = t.py[v];
    } else {
      if (v - n == self_extra) return;
      q.x = o.exy[2 * (v - n)]; q.y = o.exy[2 * (v - n) + 1];
    }
    // (integer box test first: with thousands of points almost every candidate is rejected here, without the sqrt)
    const int ix = u.x - q.x, iy = u.y - q.y;
    if (ix > mi || ix < -mi || iy > mi || iy < -mi) return;
    double dx = (double)ix, dy = (double)iy;
    double d = sqrt(dx * dx + dy * dy);
    if (d > P->max_inter) return;
    if (v < n) { q.s = t.ps[v]; q.r = t.pr[v]; q.a = t.pa[v]; }
    else { q.s = o.emarks[3 * (v - n)]; q.r = o.emarks[3 * (v - n) + 1]; q.a = o.emarks[3 * (v - n) + 2]; }
    for (int p = 0; p < M.n_pair; ++p)
      if (d <= M.pair[p].max_dist) red[p] = reduce2(M.pair[p].reduce, red[p], pair_value_rects(M.pair[p], u, gu, q, d));
  };
  if (g.start) {
    const int r = (int)ceil(P->max_inter / P->res);
    const int ci = grid_coord(P, u.x), cj = grid_coord(P, u.y);
    for (int i = max(ci - r, 0); i <= min(ci + r, P->nx - 1); ++i)
      for (int j = max(cj - r, 0); j <= min(cj + r, P->ny - 1); ++j) {
        const int c = j + i * P->ny;
        for (int k = g.start[c]; k < g.start[c + 1]; ++k) visit(g.items[k]);
      }
    for (int e = 0; e < o.n_extra; ++e) visit(n + e);
  } else {
    for (int v = 0; v < n + o.n_extra; ++v) visit(v);
  }
}

// energy vector (unit terms then pair reductions) of rectangle u in the state
// (configuration - excluded + extras); energy_graph.py:108-137
__device__ inline double point_energy(const DevParams *P, const TileRef &t, int n, const Rect &u, int self_slot,
                                      int self_extra, const Overlay &o, double *vec_or_null, const Grid &g) {
  const mpp_model &M = P->model;
  Geo gu = make_geo(u);
  double lin; int gate;
  unit_part<true>(P, t, &P->maps.edges[0][0], u, gu, &lin, &gate, vec_or_null);
  double red[MPP_MAX_PAIR] = {0.0, 0.0};
  point_reductions(P, t, n, u, gu, self_slot, self_extra, o, g, red);
  if (vec_or_null) for (int p = 0; p < M.n_pair; ++p) vec_or_null[M.n_unit + p] = red[p];
  return finish_energy(P, lin + pair_part(P, gate, red[0], red[1]));
}
