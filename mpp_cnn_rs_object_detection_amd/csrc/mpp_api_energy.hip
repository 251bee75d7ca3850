// mpp_api_energy.hip -- the from-scratch side of the C ABI (mpp_scratch.hip, mpp_maps.hip, mpp_gather.hip, mpp_metrics.hip):
// total energy, deltas, Papangelou, merge + scoring, naive initialisation, packing of detections, rotated IoU.
#include <cmath>

#include "mpp_ctx.hpp"

// Build the candidate grid of `tile` when its configuration is large enough to pay for four small launches; returns
// the two device arrays through start / items (nullptr, nullptr: the kernels scan the whole configuration).
static int scratch_grid(mpp_ctx *c, int tile, int n, const int32_t **start, const int32_t **items) {
  *start = *items = nullptr;
  if (c->grid_min_points <= 0 || n < c->grid_min_points) return 0;
  const int ncell = c->hp.nx * c->hp.ny;
  if (ncell <= 0) return 0;
  if (c->g_cells.reserve(c->stream, ((size_t)2 * ncell + 1) * sizeof(int32_t)) != hipSuccess ||
      c->g_items.reserve(c->stream, (size_t)c->cap * sizeof(int32_t)) != hipSuccess) return -2;
  int32_t *g_start = (int32_t *)c->g_cells.p;
  *start = g_start; *items = (const int32_t *)c->g_items.p;
  mpp_launch_grid_build(c->stream, c->dp, c->d_tiles, tile, n, ncell, g_start, g_start + ncell + 1, (int32_t *)c->g_items.p);
  return 0;
}

extern "C" int mpp_pack_detections(mpp_ctx *c, int n, const int32_t *tile_ids, const int32_t *anchors, int capacity,
                                   double *out_dev, int32_t *count) {
  if (!c || !c->have_maps || n <= 0 || n > c->n_tiles || !tile_ids || !anchors || capacity < 0 || !out_dev)
    return fail(c, -1, "bad pack_detections arguments");
  int rc = push_state(c);
  if (rc) return rc;
  DevBuf<int32_t> d_meta;
  HIPCHK(c, d_meta.alloc((size_t)3 * n));
  hipError_t e = hipMemcpyAsync(d_meta, tile_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_meta + n, anchors, (size_t)2 * n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(out_dev, 0, ((size_t)capacity + 1) * 7 * sizeof(double), c->stream);
  double total = 0.0;
  if (e == hipSuccess) {
    mpp_launch_pack_detections(c->stream, c->d_tiles, n, d_meta, d_meta + n, capacity, out_dev);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&total, out_dev, sizeof(double), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  if (count) *count = (int32_t)total;
  if ((int)total > capacity)
    return fail(c, -4, "%d detections exceed the gather buffer's capacity %d", (int)total, capacity);
  return 0;
}

extern "C" int mpp_total_energy(mpp_ctx *c, int tile, double *energy, double *vectors) {
  int rc = check_tile(c, tile);
  if (rc) return rc;
  if ((rc = push_state(c))) return rc;
  int32_t n = 0;
  if ((rc = mpp_count(c, tile, &n))) return rc;
  double e = 0.0;
  if (n > 0) {
    int nt = c->hp.model.n_unit + c->hp.model.n_pair;
    DevBuf<double> d_e, d_v;
    HIPCHK(c, d_e.alloc((size_t)n));
    if (vectors) HIPCHK(c, d_v.alloc((size_t)n * nt));
    const int32_t *gs, *gi;
    if (scratch_grid(c, tile, n, &gs, &gi)) return fail(c, -2, "no device memory for the candidate grid");
    mpp_launch_point_energies(c->stream, c->dp, c->d_tiles, tile, n, d_e, d_v, gs, gi);
    std::vector<double> he(n);
    hipError_t e1 = hipMemcpyAsync(he.data(), d_e, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipSuccess;
    if (vectors) e2 = hipMemcpyAsync(vectors, d_v, (size_t)n * nt * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    hipError_t e3 = hipStreamSynchronize(c->stream);
    HIPCHK(c, e1); HIPCHK(c, e2); HIPCHK(c, e3);
    for (int i = 0; i < n; ++i) e += he[i];                      // same order as the reference's np.sum over points
  }
  if (energy) *energy = e;
  return 0;
}

// mpp_total_energy of every chain of the context at once: the launches of chain_energy_launches (mpp_ctx.hpp), one copy of
// n_chains doubles and one synchronise.
extern "C" int mpp_total_energy_all(mpp_ctx *c, double *energy) {
  if (!c || !energy) return fail(c, -1, "bad total_energy_all arguments");
  int rc = push_state(c);
  if (rc) return rc;
  double *d_sum = nullptr;
  if ((rc = chain_energy_launches(c, &d_sum))) return rc;
  hipError_t e = hipMemcpyAsync(energy, d_sum, (size_t)c->n_tiles * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  return 0;
}

// The per-point energies of those launches (they start the workspace): rows of cap doubles, zero behind a chain's count.
extern "C" int mpp_point_energies_all(mpp_ctx *c, double *e) {
  if (!c || !e) return fail(c, -1, "bad point_energies_all arguments");
  int rc = push_state(c);
  if (rc) return rc;
  double *d_sum = nullptr;
  if ((rc = chain_energy_launches(c, &d_sum))) return rc;
  const int T = c->n_tiles;
  const size_t TC = (size_t)T * c->cap;
  std::vector<int32_t> n(T);
  hipError_t e0 = hipMemcpyAsync(e, c->energy_ws.p, TC * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  hipError_t e1 = hipMemcpyAsync(n.data(), c->n, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e0); HIPCHK(c, e1); HIPCHK(c, e2);
  for (int t = 0; t < T; ++t)                                   // (the kernel writes the slots below the count only)
    for (int s = n[t] < 0 ? 0 : n[t]; s < c->cap; ++s) e[(size_t)t * c->cap + s] = 0.0;
  return 0;
}

// Recombination of restarts (mpp_recombine.hip; the rules: include/mpp_hip.h): the energy launches, the tiles' kernel, the
// energy launches on the written state, one copy of the reports (and of src) and one synchronise.
extern "C" int mpp_recombine(mpp_ctx *c, mpp_recombine_report *report, int32_t *src) {
  if (!c) return -1;
  if (!c->have_maps || !c->have_model) return fail(c, -1, "recombine: mpp_set_maps / mpp_set_model have not been called");
  if (!report) return fail(c, -1, "recombine: report is NULL");
  const int R = c->replicas, T = c->n_tiles, n = c->n_maps;
  if (R < 2) return fail(c, -1, "recombine: it chooses among the replicas of a tile, \"replicas\" is %d (needs >= 2)", R);
  if (T > 65535) return fail(c, -1, "recombine: %d chains, at most 65535", T);
  for (int p = 0; p < c->hp.model.n_pair; ++p)                   // (the locality argument needs an order-free reduction)
    if (c->hp.model.pair[p].reduce != MPP_REDUCE_MAX && c->hp.model.pair[p].reduce != MPP_REDUCE_MIN)
      return fail(c, -1, "recombine: pair term %d has a reduction that is neither max nor min", p);
  int rc = push_state(c);
  if (rc) return rc;
  if (c->recombine_ws.reserve(c->stream, mpp_recombine_bytes(n, R, c->cap)) != hipSuccess)
    return fail(c, -2, "no device memory for the recombination of %d tile(s) of %d replicas", n, R);
  Recomb ws;
  mpp_recombine_plan(&ws, n, R, c->cap, c->recombine_ws.p);
  double *d_sum = nullptr;
  if ((rc = chain_energy_launches(c, &d_sum))) return rc;
  mpp_launch_recombine(c->stream, c->dp, c->d_tiles, ws, (const double *)c->energy_ws.p, d_sum, c->recombine_lds);
  if ((rc = chain_energy_launches(c, &d_sum))) return rc;
  mpp_launch_recombine_after(c->stream, ws, d_sum);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(report, ws.rep, (size_t)n * sizeof(mpp_recombine_report), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && src) e = hipMemcpyAsync(src, ws.src, (size_t)n * c->cap * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  return 0;
}

// What mpp_birth_energy_map and mpp_birth_complete refuse alike; `who` names the caller in the message.
static int birth_refusals(mpp_ctx *c, const char *who) {
  if (!c->have_maps || !c->have_model) return fail(c, -1, "%s: mpp_set_maps / mpp_set_model have not been called", who);
  if (model_class(c->hp).classic)
    return fail(c, -1, "%s: the model has a classic image energy (a candidate per pixel would need a rasterised "
                       "footprint per pixel)", who);
  return 0;
}
// The launches of one birth-energy map of every chain (mpp_birth_map.hip): grids as mpp_total_energy_all builds them, the
// pre-pass that caches every point's record, the map.  After push_state; part / d_sum: the summary's workspace.
static int birth_map_launches(mpp_ctx *c, const char *who, double *dE, double *marks, BirthPart **part, mpp_birth_summary **d_sum) {
  const int T = c->n_tiles;
  if (T > 65535) return fail(c, -1, "%s: %d chains, at most 65535", who, T);
  const size_t TC = (size_t)T * c->cap;
  // doubles: lin, r0, r1, e [T][cap]; the summary's parts and results; ints: gate [T][cap]
  const size_t part_bytes = (size_t)T * MPP_BIRTH_PARTS * sizeof(BirthPart), sum_bytes = (size_t)T * sizeof(mpp_birth_summary);
  ChainGrids g;
  if (c->birth_ws.reserve(c->stream, 4 * TC * sizeof(double) + part_bytes + sum_bytes + TC * sizeof(int32_t)) != hipSuccess ||
      chain_grids_build(c, c->cap, chain_grids_on(c), &g))
    return fail(c, -2, "no device memory for the point cache of %d chains", T);
  double *d0 = (double *)c->birth_ws.p;
  *part = (BirthPart *)(d0 + 4 * TC);
  *d_sum = (mpp_birth_summary *)(*part + (size_t)T * MPP_BIRTH_PARTS);
  const BirthCache bc{d0, d0 + TC, d0 + 2 * TC, d0 + 3 * TC, (int32_t *)(*d_sum + T)};
  c->birth_grid = g.ncell > 0 ? 1 : 0;
  mpp_launch_birth_prepass(c->stream, c->dp, c->d_tiles, T, c->cap, bc, g.start, g.items, g.ncell + 1, c->grid_min_points);
  mpp_launch_birth_map(c->stream, c->dp, c->d_tiles, T, c->cap, c->H, c->W, bc, dE, marks);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The birth-energy map of every chain, and -- when asked for -- the summary, whose copy back is the call's only wait.
extern "C" int mpp_birth_energy_map(mpp_ctx *c, double *dE, double *marks, mpp_birth_summary *summary) {
  if (!c) return -1;
  int rc = birth_refusals(c, "birth_energy_map");
  if (rc) return rc;
  if (!dE) return fail(c, -1, "birth_energy_map: dE is NULL");
  if ((rc = push_state(c))) return rc;
  BirthPart *part;
  mpp_birth_summary *d_sum;
  if ((rc = birth_map_launches(c, "birth_energy_map", dE, marks, &part, &d_sum))) return rc;
  if (summary) {
    const int T = c->n_tiles;
    mpp_launch_birth_summary(c->stream, T, c->H, c->W, dE, part, d_sum);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(summary, d_sum, (size_t)T * sizeof(mpp_birth_summary), hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    HIPCHK(c, e); HIPCHK(c, e2);
  }
  return 0;
}

// The first block of a selection and its workspace (mpp_birth_complete.hip)
static int minsel_setup(mpp_ctx *c, MinSel *s, const double *dE, size_t chain_stride, int T, int H, int W, int ld, double below,
                        double distance, const mpp_descent_report *rep) {
  *s = MinSel{};
  s->dE = dE; s->chain_stride = chain_stride; s->H = H; s->W = W; s->ld = ld; s->n_chains = T;
  s->below = below; s->d2 = distance * distance;
  const double side = (double)(H > W ? H : W);
  s->reach = (int)floor(distance < side ? distance + 1.0 : side);     // (one more than floor(distance): the test itself is d2's)
  s->rep = rep;
  if (c->minsel_ws.reserve(c->stream, mpp_minsel_bytes(T, H, W)) != hipSuccess)
    return fail(c, -2, "no device memory for the candidate list of %d map(s) of %d x %d", T, H, W);
  mpp_minsel_plan(s, c->minsel_ws.p);
  return 0;
}

extern "C" int mpp_select_minima(mpp_ctx *c, int H, int W, int ld, const double *dE, double below, double distance, int cap,
                                 int32_t *xy, double *values, int64_t *n_candidates, int64_t *n_kept) {
  if (!c) return -1;
  if (H < 1 || W < 1 || ld < W || !dE || cap < 0 || (cap > 0 && (!xy || !values)) || !(distance >= 0.0) || !std::isfinite(distance) ||
      !std::isfinite(below) || (long long)H * W >= (1ll << 31))
    return fail(c, -1, "bad select_minima arguments");
  HIPCHK(c, hipSetDevice(c->device));
  MinSel s;
  int rc = minsel_setup(c, &s, dE, 0, 1, H, W, ld, below, distance, nullptr);
  if (rc) return rc;
  mpp_launch_minsel(c->stream, s);
  hipError_t e = hipGetLastError();
  int32_t n[2] = {0, 0};                                   // (n_cand and n_kept lie side by side for one chain)
  if (e == hipSuccess) e = hipMemcpyAsync(n, s.n_cand, sizeof n, hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  if (n_candidates) *n_candidates = n[0];
  if (n_kept) *n_kept = n[1];
  if (n[1] > cap) return fail(c, -13, "select_minima: %d minima kept, the output holds %d", n[1], cap);
  if (n[1] > 0) {
    mpp_launch_minsel_emit(c->stream, s, cap, xy, values);
    e = hipGetLastError();
    e2 = hipStreamSynchronize(c->stream);
    HIPCHK(c, e); HIPCHK(c, e2);
  }
  return 0;
}

// ---- the local descent (mpp_descent.hip) -------------------------------------------------------------------
// The launches of mpp_merge_score's scoring for every chain, into p [n_chains][cap]; the counts stay on the device (a block per
// slot of the capacity: the blocks behind a chain's count return at once).  k_papangelou_tiles has no threshold per chain, so
// with the grids on every chain uses its own; the values are the same bits either way.  `what` names the caller's workspace.
static int papangelou_launches(mpp_ctx *c, double *p, const char *what) {
  ChainGrids g;
  if (chain_grids_build(c, c->cap, chain_grids_on(c), &g))
    return fail(c, -2, "no device memory for the %s of %d chains", what, c->n_tiles);
  mpp_launch_papangelou_tiles(c->stream, c->dp, c->d_tiles, c->n_tiles, c->cap, c->cap, p, g.start, g.items, g.ncell + 1, c->cap);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" int mpp_papangelou_all(mpp_ctx *c, double *dE) {
  if (!c || !dE) return fail(c, -1, "bad papangelou_all arguments");
  int rc = push_state(c);
  if (rc) return rc;
  const int T = c->n_tiles;
  if (T > 65535) return fail(c, -1, "papangelou_all: %d chains, at most 65535", T);
  if (c->descent_ws.reserve(c->stream, mpp_descent_bytes(T, c->cap, 0)) != hipSuccess)
    return fail(c, -2, "no device memory for the Papangelou values of %d chains", T);
  Descent d;
  mpp_descent_plan(&d, T, c->cap, 0, c->descent_ws.p);
  const size_t bytes = (size_t)T * c->cap * sizeof(double);
  HIPCHK(c, hipMemsetAsync(d.p, 0, bytes, c->stream));           // (the kernel writes the slots below a chain's count only)
  if ((rc = papangelou_launches(c, d.p, "Papangelou values"))) return rc;
  hipError_t e = hipMemcpyAsync(dE, d.p, bytes, hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  return 0;
}

extern "C" int mpp_select_points(mpp_ctx *c, int n, const int32_t *xy, const double *values, double above, double distance,
                                 uint8_t *keep, int64_t *n_candidates, int64_t *n_kept) {
  if (!c) return -1;
  if (n < 0 || (n > 0 && (!xy || !values || !keep)) || !(distance >= 0.0) || !std::isfinite(distance) || !std::isfinite(above))
    return fail(c, -1, "bad select_points arguments");
  HIPCHK(c, hipSetDevice(c->device));
  int32_t count[2] = {0, 0};
  if (n > 0) {
    if (c->ptsel_ws.reserve(c->stream, sizeof count) != hipSuccess) return fail(c, -2, "no device memory for select_points");
    PtSel s{};
    s.n_chains = 1; s.x = xy; s.y = xy + 1; s.stride = 2; s.n = n; s.val = values; s.keep = keep;
    s.above = above; s.d2 = distance * distance; s.count = (int32_t *)c->ptsel_ws.p;
    HIPCHK(c, hipMemsetAsync(s.count, 0, sizeof count, c->stream));
    mpp_launch_ptsel(c->stream, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(count, s.count, sizeof count, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    HIPCHK(c, e); HIPCHK(c, e2);
  }
  if (n_candidates) *n_candidates = count[0];
  if (n_kept) *n_kept = count[1];
  return 0;
}

// The rounds of mpp_descend and of mpp_birth_complete (what = births: DESIGN.md sections 13 and 16), from the refusal of too many
// chains to the round that closes the last chain.  Per round: the launches of the Papangelou pass, of the selection among
// points and of the removal; those of the map, of the selection of its minima and of their append; the round's book (the one
// record a chain has, its descent report); one copy of the chains' reports to report [n_chains].  The point lists and the maps
// stay on the device.  `who` names the caller and `noun` its workspace in the messages.  Then the tail: the Papangelou values
// and the map of the returned state, each recomputed only when the last one is not that state's, and their summaries.  The
// completion (values = false) takes neither a Papangelou pass nor a value of d.p, which nothing has filled for it.
static int descent_rounds(mpp_ctx *c, const char *who, const char *noun, int what, bool values, int max_rounds, double min_gain,
                          mpp_descent_report *report, int32_t *src) {
  const bool deaths = what & MPP_DESCEND_DEATHS, births = what & MPP_DESCEND_BIRTHS;
  const int T = c->n_tiles, H = c->H, W = c->W;
  if (T > 65535) return fail(c, -1, "%s: %d chains, at most 65535", who, T);
  int rc = push_state(c);
  if (rc) return rc;
  const size_t hw = births ? (size_t)H * W : 0;
  if (c->descent_ws.reserve(c->stream, mpp_descent_bytes(T, c->cap, hw)) != hipSuccess)
    return fail(c, -2, "no device memory for the %s of %d chains", noun, T);
  Descent d;
  mpp_descent_plan(&d, T, c->cap, hw, c->descent_ws.p);
  const double reach = 2.0 * c->hp.max_inter;
  MinSel s{};
  if (births && (rc = minsel_setup(c, &s, d.dE, hw, T, H, W, W, -min_gain, reach, d.rep))) return rc;
  PtSel ps{};
  ps.tiles = c->d_tiles; ps.n_chains = T; ps.cap = c->cap; ps.val = d.p; ps.keep = d.keep; ps.pitch = (size_t)c->cap;
  ps.above = min_gain; ps.d2 = reach * reach; ps.closed = d.rep;
  mpp_launch_descent_init(c->stream, c->d_tiles, d);
  BirthPart *part = nullptr;
  mpp_birth_summary *d_sum = nullptr;
  bool stale_p = !deaths, stale_map = false, open = true;
  std::vector<int32_t> was(T, -1);
  // (a chain is open for at most max_rounds rounds that change it and the one that closes it)
  for (int round = 0; round <= max_rounds && open; ++round) {
    if (deaths) {
      if ((rc = papangelou_launches(c, d.p, noun))) return rc;
      mpp_launch_ptsel(c->stream, ps);
      mpp_launch_descent_remove(c->stream, c->d_tiles, d);
    }
    if (births) {
      if ((rc = birth_map_launches(c, who, d.dE, nullptr, &part, &d_sum))) return rc;
      mpp_launch_minsel(c->stream, s);
      mpp_launch_complete_append(c->stream, s, c->dp, c->d_tiles, c->cap, d.gain_val);
    }
    mpp_launch_descent_round(c->stream, c->d_tiles, d, what, max_rounds, s.n_kept);   // (s.n_kept: nullptr without births)
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(report, d.rep, (size_t)T * sizeof(mpp_descent_report), hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    HIPCHK(c, e); HIPCHK(c, e2);
    open = false;
    for (int t = 0; t < T; ++t) {
      const int st = report[t].status;
      open = open || st < 0;
      // a chain that changed in the round that closed it: its last Papangelou values (its last map) are not its state's
      if (was[t] < 0 && st > 0) { stale_p = true; stale_map = stale_map || st == 1; }
      was[t] = st;
    }
  }
  if (open) return fail(c, -9, "%s: a chain is still open after %d rounds", who, max_rounds + 1);
  if (!values) d.p = nullptr;                                    // (k_descent_summary then skips its reduction)
  else if (stale_p && (rc = papangelou_launches(c, d.p, noun))) return rc;
  if (births) {
    if (stale_map && (rc = birth_map_launches(c, who, d.dE, nullptr, &part, &d_sum))) return rc;
    mpp_launch_birth_summary(c->stream, T, H, W, d.dE, part, d_sum);
  }
  mpp_launch_descent_summary(c->stream, c->d_tiles, d, d_sum);   // (d_sum: nullptr without births)
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(report, d.rep, (size_t)T * sizeof(mpp_descent_report), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && src) e = hipMemcpyAsync(src, d.src, (size_t)T * c->cap * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  return 0;
}

// What mpp_birth_complete and mpp_descend refuse alike in their round limit and gain
static int rounds_refusals(mpp_ctx *c, const char *who, int max_rounds, double min_gain) {
  if (max_rounds < 1 || max_rounds > 1024) return fail(c, -1, "%s: max_rounds %d, must be 1..1024", who, max_rounds);
  if (!(min_gain >= 0.0) || !std::isfinite(min_gain)) return fail(c, -1, "%s: min_gain must be finite and >= 0", who);
  return 0;
}

// Greedy completion: the births-only form of the descent, without its Papangelou values; the caller's
// records are filled from the chains' descent reports.
extern "C" int mpp_birth_complete(mpp_ctx *c, int max_rounds, double min_gain, mpp_complete_report *report) {
  if (!c) return -1;
  int rc = birth_refusals(c, "birth_complete");
  if (rc) return rc;
  if (!report) return fail(c, -1, "birth_complete: report is NULL");
  if ((rc = rounds_refusals(c, "birth_complete", max_rounds, min_gain))) return rc;
  const int T = c->n_tiles;
  std::vector<mpp_descent_report> book(T > 0 ? T : 1);
  if ((rc = descent_rounds(c, "birth_complete", "maps", MPP_DESCEND_BIRTHS, false, max_rounds, min_gain, book.data(), nullptr)))
    return rc;
  for (int t = 0; t < T; ++t) {
    const mpp_descent_report &b = book[t];
    report[t] = mpp_complete_report{b.status, b.rounds, b.n_added, b.n_after, b.gain_births, b.min_dE, b.x, b.y, b.n_negative, b.n_nan};
  }
  return 0;
}

extern "C" int mpp_descend(mpp_ctx *c, int what, int max_rounds, double min_gain, mpp_descent_report *report, int32_t *src) {
  if (!c) return -1;
  if (what < 1 || what > 3) return fail(c, -1, "descend: what %d, must be 1 (deaths), 2 (births) or 3 (both)", what);
  const bool births = what & MPP_DESCEND_BIRTHS;
  int rc = 0;
  if (births) { if ((rc = birth_refusals(c, "descend"))) return rc; }
  else if (!c->have_maps || !c->have_model) return fail(c, -1, "descend: mpp_set_maps / mpp_set_model have not been called");
  if (!report) return fail(c, -1, "descend: report is NULL");
  if ((rc = rounds_refusals(c, "descend", max_rounds, min_gain))) return rc;
  for (int p = 0; p < c->hp.model.n_pair; ++p)                   // (a round's gains add up only under an order-free reduction)
    if (c->hp.model.pair[p].reduce != MPP_REDUCE_MAX && c->hp.model.pair[p].reduce != MPP_REDUCE_MIN)
      return fail(c, -1, "descend: pair term %d has a reduction that is neither max nor min", p);
  return descent_rounds(c, "descend", "descent", what, true, max_rounds, min_gain, report, src);
}

// ---- relocation (mpp_relocate.hip) --------------------------------------------------------------------------
// What mpp_move_gains and mpp_relocate refuse alike; `who` names the caller in the message.
static int move_refusals(mpp_ctx *c, const char *who, int radius) {
  if (radius < 1 || radius > MPP_MOVE_RADIUS_MAX)
    return fail(c, -1, "%s: radius %d, must be 1..%d", who, radius, MPP_MOVE_RADIUS_MAX);
  int rc = birth_refusals(c, who);
  if (rc) return rc;
  for (int p = 0; p < c->hp.model.n_pair; ++p)                   // (a reduction without its best contributor needs a selection)
    if (c->hp.model.pair[p].reduce != MPP_REDUCE_MAX && c->hp.model.pair[p].reduce != MPP_REDUCE_MIN)
      return fail(c, -1, "%s: pair term %d has a reduction that is neither max nor min", who, p);
  if (c->n_tiles > 65535) return fail(c, -1, "%s: %d chains, at most 65535", who, c->n_tiles);
  return 0;
}
// The two workspaces of a call, after push_state: the Descent's (the gains in d->p, the selection's answer, the round's list,
// the closed flags) and the Move's.
static int move_setup(mpp_ctx *c, const char *who, Descent *d, Move *m) {
  const int T = c->n_tiles;
  if (c->descent_ws.reserve(c->stream, mpp_descent_bytes(T, c->cap, 0)) != hipSuccess ||
      c->relocate_ws.reserve(c->stream, mpp_move_bytes(T, c->cap)) != hipSuccess)
    return fail(c, -2, "%s: no device memory for the move gains of %d chains", who, T);
  mpp_descent_plan(d, T, c->cap, 0, c->descent_ws.p);
  mpp_move_plan(m, T, c->cap, c->relocate_ws.p);
  return 0;
}
// The launches of one gain pass over every chain (or every open one): grids as mpp_total_energy_all builds them, the pre-pass, the gains
static int move_gain_launches(mpp_ctx *c, const char *who, int radius, const Move &m, const Descent &d, bool skip_closed) {
  ChainGrids g;
  if (chain_grids_build(c, c->cap, chain_grids_on(c), &g))
    return fail(c, -2, "%s: no device memory for the candidate grids of %d chains", who, c->n_tiles);
  c->move_grid = g.ncell > 0 ? 1 : 0;
  mpp_launch_move_gains(c->stream, c->dp, c->d_tiles, m, d, radius, g.start, g.items, g.ncell + 1, c->grid_min_points, skip_closed ? 1 : 0);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" int mpp_move_gains(mpp_ctx *c, int radius, double *gain, int32_t *to) {
  if (!c) return -1;
  int rc = move_refusals(c, "move_gains", radius);
  if (rc) return rc;
  if (!gain || !to) return fail(c, -1, "move_gains: gain or to is NULL");
  if ((rc = push_state(c))) return rc;
  Descent d;
  Move m;
  if ((rc = move_setup(c, "move_gains", &d, &m))) return rc;
  const size_t TC = (size_t)c->n_tiles * c->cap;
  HIPCHK(c, hipMemsetAsync(d.p, 0, TC * sizeof(double), c->stream));         // (the kernel writes the slots below a chain's count only)
  HIPCHK(c, hipMemsetAsync(m.to, 0xff, 2 * TC * sizeof(int32_t), c->stream));
  if ((rc = move_gain_launches(c, "move_gains", radius, m, d, false))) return rc;
  hipError_t e = hipMemcpyAsync(gain, d.p, TC * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(to, m.to, 2 * TC * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  return 0;
}

// The rounds of mpp_relocate.  Per round: the launches of the gain pass, of the selection among points, of the rewrite and of
// the round's book; one copy of the chains' books to report [n_chains].  Then the tail: the gains of the returned state,
// recomputed when a chain moved in the round that closed it, and their summary.
extern "C" int mpp_relocate(mpp_ctx *c, int radius, int max_rounds, double min_gain, mpp_relocate_report *report, int32_t *moved) {
  if (!c) return -1;
  int rc = move_refusals(c, "relocate", radius);
  if (rc) return rc;
  if (!report) return fail(c, -1, "relocate: report is NULL");
  if ((rc = rounds_refusals(c, "relocate", max_rounds, min_gain))) return rc;
  if ((rc = push_state(c))) return rc;
  Descent d;
  Move m;
  if ((rc = move_setup(c, "relocate", &d, &m))) return rc;
  const int T = c->n_tiles;
  const size_t TC = (size_t)T * c->cap;
  const double distance = 2.0 * (c->hp.max_inter + (double)radius * sqrt(2.0));
  PtSel ps{};
  ps.tiles = c->d_tiles; ps.n_chains = T; ps.cap = c->cap; ps.val = d.p; ps.keep = d.keep; ps.pitch = (size_t)c->cap;
  ps.above = min_gain; ps.d2 = distance * distance; ps.closed = d.rep;
  HIPCHK(c, hipMemsetAsync(m.moved, 0, TC * sizeof(int32_t), c->stream));
  HIPCHK(c, hipMemsetAsync(m.to, 0xff, 2 * TC * sizeof(int32_t), c->stream));
  mpp_launch_descent_init(c->stream, c->d_tiles, d);
  mpp_launch_move_init(c->stream, c->d_tiles, m);
  bool stale = false, open = T > 0;
  // (a chain is open for at most max_rounds rounds that move something and the one that closes it)
  for (int round = 0; round <= max_rounds && open; ++round) {
    if ((rc = move_gain_launches(c, "relocate", radius, m, d, true))) return rc;
    mpp_launch_ptsel(c->stream, ps);
    mpp_launch_move_apply(c->stream, c->dp, c->d_tiles, m, d);
    mpp_launch_move_round(c->stream, c->d_tiles, m, d, max_rounds);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(report, m.rep, (size_t)T * sizeof(mpp_relocate_report), hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    HIPCHK(c, e); HIPCHK(c, e2);
    open = false;
    for (int t = 0; t < T; ++t) {
      open = open || report[t].status < 0;
      stale = stale || report[t].status == 1;                    // (moved in the round that closed it: its gains are not its state's)
    }
  }
  if (open) return fail(c, -9, "relocate: a chain is still open after %d rounds", max_rounds + 1);
  if (stale && (rc = move_gain_launches(c, "relocate", radius, m, d, false))) return rc;
  mpp_launch_descent_summary(c->stream, c->d_tiles, d, nullptr);
  mpp_launch_move_finish(c->stream, m, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(report, m.rep, (size_t)T * sizeof(mpp_relocate_report), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && moved) e = hipMemcpyAsync(moved, m.moved, TC * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  return 0;
}

// shared body of mpp_delta_batch (dE != NULL) and mpp_delta_vectors (before/after/mask != NULL)
static int delta_cases(mpp_ctx *c, int tile, int n_cases, const int32_t *rem_off, const int32_t *rem,
                       const int32_t *add_off, const int32_t *add_xy, const double *add_marks, double *dE, int stride,
                       double *before, double *after, unsigned char *mask) {
  int rc = check_tile(c, tile);
  if (rc) return rc;
  if ((rc = push_state(c))) return rc;
  if (n_cases <= 0) return 0;
  int32_t n = 0;
  if ((rc = mpp_count(c, tile, &n))) return rc;
  const int n_rem = rem_off[n_cases], n_add = add_off[n_cases];
  for (int i = 0; i < n_rem; ++i)
    if (rem[i] < 0 || rem[i] >= n) return fail(c, -6, "removal of slot %d: no such point (n=%d)", rem[i], n);  // KeyError
  for (int i = 0; i < n_add; ++i)
    if (add_xy[2 * i] < 0 || add_xy[2 * i] >= c->H || add_xy[2 * i + 1] < 0 || add_xy[2 * i + 1] >= c->W)
      return fail(c, -5, "added point %d is outside the tile", i);
  const int nt = c->hp.model.n_unit + c->hp.model.n_pair;
  if (!dE) {
    for (int i = 0; i < n_cases; ++i)
      if (n + (add_off[i + 1] - add_off[i]) > stride)
        return fail(c, -1, "delta_vectors: stride %d < n + additions of case %d (%d)", stride, i, n + add_off[i + 1] - add_off[i]);
  }
  const int32_t *gs, *gi;
  if (scratch_grid(c, tile, n, &gs, &gi)) return fail(c, -2, "no device memory for the candidate grid");
  DevBuf<int32_t> d_ro, d_r, d_ao, d_axy;
  DevBuf<double> d_am, d_out, d_b, d_a;
  DevBuf<unsigned char> d_m;
  const size_t rows = dE ? 0 : (size_t)n_cases * stride;
  HIPCHK(c, d_ro.alloc((size_t)n_cases + 1)); HIPCHK(c, d_ao.alloc((size_t)n_cases + 1));
  HIPCHK(c, d_r.alloc((size_t)n_rem)); HIPCHK(c, d_axy.alloc((size_t)2 * n_add));
  HIPCHK(c, d_am.alloc((size_t)3 * n_add));
  if (dE) HIPCHK(c, d_out.alloc((size_t)n_cases));
  else { HIPCHK(c, d_b.alloc(rows * nt)); HIPCHK(c, d_a.alloc(rows * nt)); HIPCHK(c, d_m.alloc(rows)); }
  hipError_t e = hipSuccess;
  auto up = [&](void *dst, const void *src, size_t bytes) {
    if (bytes && e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
  };
  up(d_ro, rem_off, (n_cases + 1) * sizeof(int32_t)); up(d_ao, add_off, (n_cases + 1) * sizeof(int32_t));
  up(d_r, rem, n_rem * sizeof(int32_t)); up(d_axy, add_xy, 2 * (size_t)n_add * sizeof(int32_t));
  up(d_am, add_marks, 3 * (size_t)n_add * sizeof(double));
  if (e == hipSuccess) {
    if (dE) {
      mpp_launch_delta_batch(c->stream, c->dp, c->d_tiles, tile, n_cases, d_ro, d_r, d_ao, d_axy, d_am, d_out, gs, gi);
      e = hipMemcpyAsync(dE, d_out, n_cases * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    } else {
      mpp_launch_delta_vectors(c->stream, c->dp, c->d_tiles, tile, n_cases, d_ro, d_r, d_ao, d_axy, d_am, stride, d_b, d_a, d_m, gs, gi);
      e = hipMemcpyAsync(before, d_b, rows * nt * sizeof(double), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(after, d_a, rows * nt * sizeof(double), hipMemcpyDeviceToHost, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(mask, d_m, rows, hipMemcpyDeviceToHost, c->stream);
    }
  }
  hipError_t e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  return 0;
}

extern "C" int mpp_delta_batch(mpp_ctx *c, int tile, int n_cases, const int32_t *rem_off, const int32_t *rem,
                               const int32_t *add_off, const int32_t *add_xy, const double *add_marks, double *dE) {
  if (!dE && n_cases > 0) return fail(c, -1, "delta_batch: dE is NULL");
  return delta_cases(c, tile, n_cases, rem_off, rem, add_off, add_xy, add_marks, dE, 0, nullptr, nullptr, nullptr);
}
extern "C" int mpp_delta_vectors(mpp_ctx *c, int tile, int n_cases, const int32_t *rem_off, const int32_t *rem,
                                 const int32_t *add_off, const int32_t *add_xy, const double *add_marks, int stride,
                                 double *before, double *after, unsigned char *mask) {
  if (n_cases > 0 && (!before || !after || !mask || stride <= 0)) return fail(c, -1, "bad delta_vectors arguments");
  return delta_cases(c, tile, n_cases, rem_off, rem, add_off, add_xy, add_marks, nullptr, stride, before, after, mask);
}

extern "C" int mpp_papangelou(mpp_ctx *c, int tile, double *dE) {
  int32_t n = 0;
  int rc = mpp_count(c, tile, &n);
  if (rc) return rc;
  if (n == 0) return 0;
  std::vector<int32_t> ro(n + 1), r(n), ao(n + 1, 0);
  for (int i = 0; i <= n; ++i) ro[i] = i;
  for (int i = 0; i < n; ++i) r[i] = i;
  int32_t dummy_xy[2] = {0, 0};
  double dummy_m[3] = {0, 0, 0};
  rc = mpp_delta_batch(c, tile, n, ro.data(), r.data(), ao.data(), dummy_xy, dummy_m, dE);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) dE[i] = -dE[i];     // E(with u) - E(without u), energy_point_set.py:108-110
  return 0;
}

// merge_patches(method='distance') for every tile of the ctx at once (data_loaders.py:122-161): each tile holds the
// aggregated detections of one image on that image's score maps.  Papangelou of every point, the dedupe walk, the
// removals (EPointsSet.remove order), Papangelou of the survivors -- four launches for the whole batch, one copy back.
#define MPP_MERGE_MAX_POINTS 8192
extern "C" int mpp_merge_score(mpp_ctx *c, double distance, int cap, int32_t *n_out, int32_t *xy, double *marks, double *dE,
                               int32_t *n_removed) {
  if (!c || !n_out || cap < 0 || !(distance >= 0)) return fail(c, -1, "bad merge_score arguments");
  if (!c->have_maps || !c->have_model) return fail(c, -1, "mpp_set_maps / mpp_set_model have not been called");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = push_state(c);
  if (rc) return rc;
  const int T = c->n_tiles;
  std::vector<int32_t> n0(T);
  HIPCHK(c, hipMemcpyAsync(n0.data(), c->n, sizeof(int32_t) * T, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int max_n = 0;
  for (int t = 0; t < T; ++t) max_n = n0[t] > max_n ? n0[t] : max_n;
  if (max_n > MPP_MERGE_MAX_POINTS || (size_t)((c->cap + 7) & ~7) * 17 > (size_t)MPP_DEDUPE_LDS_MAX)      // (the walk's working set lives in LDS)
    return fail(c, -4, "merge_score: a tile holds %d points (the device walk takes at most %d): merge it on the host", max_n,
                MPP_MERGE_MAX_POINTS);
  // (the walk carries a position as two 16-bit halves; mpp_set_maps is the guard: it takes no side above 65535)
  const size_t TC = (size_t)T * c->cap;
  DevBuf<double> d_dE, ts, tr, ta;
  DevBuf<int32_t> work, slot_of, tx, ty, d_rem;
  hipError_t e = hipSuccess;
  auto A = [&](auto &buf, size_t count) { if (e == hipSuccess) e = buf.alloc(count); };
  A(d_dE, TC); A(ts, TC); A(tr, TC); A(ta, TC);
  A(work, TC); A(slot_of, TC); A(tx, TC); A(ty, TC); A(d_rem, (size_t)T);
  std::vector<int32_t> h_rem(T, 0);
  if (e == hipSuccess && max_n > 0) {
    // (64 bits: 65535^2 + 65535^2 does not fit an int; beyond that every pair of points is within the distance)
    const long long dist2 = (long long)floor(fmin(distance * distance + 1e-9, 1e10));
    // the from-scratch energies look their neighbours up in the chains' candidate grids where they pay, built on the device
    // before each of the two scorings (the removals in between move points)
    const bool grid = c->hp.nx * c->hp.ny > 0 && max_n >= 64;
    ChainGrids g;
    for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
      if (chain_grids_build(c, max_n, grid, &g)) { e = hipErrorOutOfMemory; break; }
      mpp_launch_papangelou_tiles(c->stream, c->dp, c->d_tiles, T, max_n, c->cap, d_dE, g.start, g.items, g.ncell + 1, c->cap);
      if (pass == 0) mpp_launch_dedupe_tiles(c->stream, c->d_tiles, T, max_n, c->cap, d_dE, dist2, work, slot_of, tx, ty, ts, tr, ta, d_rem);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_rem.data(), d_rem, sizeof(int32_t) * T, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  }
  if (e == hipSuccess) rc = mpp_get_points_all(c, cap, n_out, xy, marks);
  if (e == hipSuccess && rc == 0 && dE && cap > 0 && max_n > 0) {
    const int m = max_n < cap ? max_n : cap;
    std::vector<double> h((size_t)T * m);
    e = hipMemcpy2D(h.data(), (size_t)m * 8, d_dE, (size_t)c->cap * 8, (size_t)m * 8, T, hipMemcpyDeviceToHost);
    for (int t = 0; t < T && e == hipSuccess; ++t)
      for (int i = 0; i < n_out[t] && i < m; ++i) dE[(size_t)t * cap + i] = h[(size_t)t * m + i];
  }
  if (n_removed) for (int t = 0; t < T; ++t) n_removed[t] = h_rem[t];
  HIPCHK(c, e);
  return rc;
}

extern "C" int mpp_naive_init(mpp_ctx *c, double threshold, double nms_distance) {
  if (!c) return -1;
  int rc = push_state(c);
  if (rc) return rc;
  const int cand_cap = c->H * c->W;
  DevBuf<unsigned long long> cand;
  HIPCHK(c, cand.alloc((size_t)c->n_tiles * cand_cap));
  mpp_launch_naive_init(c->stream, c->dp, c->d_tiles, c->n_tiles, threshold, nms_distance, cand, cand_cap);
  hipError_t e = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  HIPCHK(c, e); HIPCHK(c, e2);
  std::vector<int32_t> herr(c->n_tiles);
  HIPCHK(c, hipMemcpy(herr.data(), c->errd, c->n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int t = 0; t < c->n_tiles; ++t)
    if (herr[t]) return fail(c, -10 - herr[t], "naive init, tile %d: %s", t, chain_error_text(herr[t]));
  return 0;
}

extern "C" int mpp_quad_iou(mpp_ctx *c, int n, const double *a, int m, const double *b, double *out, int on_device) {
  if (!c || n < 0 || m < 0 || ((long long)n * m > 0 && (!a || !b || !out))) return fail(c, -1, "bad quad_iou arguments");
  if ((long long)n * m == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  if (on_device) {
    mpp_launch_quad_iou(c->stream, n, a, m, b, out);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  DevBuf<double> da, db, dout;
  const size_t sa = (size_t)n * 8 * sizeof(double), sb = (size_t)m * 8 * sizeof(double), so = (size_t)n * m * sizeof(double);
  if (da.alloc((size_t)n * 8) != hipSuccess || db.alloc((size_t)m * 8) != hipSuccess || dout.alloc((size_t)n * m) != hipSuccess)
    return fail(c, -2, "quad_iou: device allocation failed");
  if (hipMemcpyAsync(da, a, sa, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(db, b, sb, hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(c, -2, "quad_iou: upload failed");
  mpp_launch_quad_iou(c->stream, n, da, m, db, dout);
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out, dout, so, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, -2, "quad_iou: kernel or download failed");
  return 0;
}
