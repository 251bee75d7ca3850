// mpp_api_chain.hip -- the chains of the C ABI (mpp_run, mpp_replay): birth and remap tables, the birth pre-pass, and
// run_chain, which routes every chain to the LDS or the device-memory kernel and grows the capacities until all are done.
#include <cmath>

#include "mpp_ctx.hpp"

// More slots per tile: the five configuration arrays are re-allocated with the new stride and copied.
static int grow_points(mpp_ctx *c, int new_cap) {
  const size_t T = (size_t)c->n_tiles;
  DevBuf<int32_t> px, py;
  DevBuf<double> ps, pr, pa;
  HIPCHK(c, px.alloc(T * new_cap)); HIPCHK(c, py.alloc(T * new_cap));
  HIPCHK(c, ps.alloc(T * new_cap)); HIPCHK(c, pr.alloc(T * new_cap)); HIPCHK(c, pa.alloc(T * new_cap));
  const size_t wi = (size_t)c->cap * sizeof(int32_t), wd = (size_t)c->cap * sizeof(double);
  const size_t ni = (size_t)new_cap * sizeof(int32_t), nd = (size_t)new_cap * sizeof(double);
  HIPCHK(c, hipMemcpy2DAsync(px, ni, c->px, wi, wi, T, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(py, ni, c->py, wi, wi, T, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(ps, nd, c->ps, wd, wd, T, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(pr, nd, c->pr, wd, wd, T, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(pa, nd, c->pa, wd, wd, T, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::swap(c->px, px); std::swap(c->py, py); std::swap(c->ps, ps); std::swap(c->pr, pr); std::swap(c->pa, pa);   // (the old arrays go with this scope)
  c->cap = new_cap;
  c->tiles_dirty = true; c->params_dirty = true;
  return 0;
}

// A chain evaluates MPP_U_SHAPE_REMAP -- three sigmoids of mark probabilities -- for every proposal that adds a rectangle
// (~10 % of its vector instructions).  The reference builds the remapped maps once per tile
// (energy_setup_legacy.py:142-147); so do chains here: [H][W][32] float64 per mark, holding exactly the summands the
// inline code forms (same expression, same device exp: the chain is byte-identical with and without the tables).  Only
// for models whose sole use of the mark maps is that term, only for contexts that run chains (the from-scratch energies of
// EPointsSet evaluate a few thousand points: inline), and only while 3 x 8 B x 32 per pixel fits the budget (2 GB).
static int ensure_remap_tables(mpp_ctx *c) {
  if (!c->remap_dirty) return 0;
  c->remap_dirty = false;
  const mpp_model &M = c->hp.model;
  int term = -1;
  bool other_mark_use = false;
  for (int k = 0; k < M.n_unit; ++k) {
    if (M.unit[k].kind == MPP_U_SHAPE_REMAP) term = term < 0 ? k : -2;
    if (M.unit[k].kind == MPP_U_MARK_NEG || M.unit[k].kind == MPP_U_MARK_REMAP) other_mark_use = true;
  }
  const size_t n = (size_t)c->n_maps * c->H * c->W * MPP_NCLASS, bytes = 3 * n * sizeof(double);
  const bool want = c->remap_mode != 0 && term >= 0 && !other_mark_use && (c->remap_mode == 1 || bytes <= c->remap_budget);
  if (!want) {
    if (c->remap[0]) {
      for (int k = 0; k < 3; ++k) c->remap[k].reset();
      c->tiles_dirty = true;
    }
    return 0;
  }
  for (int k = 0; k < 3; ++k) {
    if (!c->remap[k] && c->remap[k].alloc(n) != hipSuccess) {
      (void)hipGetLastError();                          // no room: chains evaluate the sigmoids inline (same values)
      for (int j = 0; j < 3; ++j) c->remap[j].reset();
      c->tiles_dirty = true;
      return 0;
    }
    mpp_launch_remap_table(c->stream, c->m[k], n, M.unit[term].p[k], M.unit[term].p[3 + k], c->remap[k]);
  }
  HIPCHK(c, hipGetLastError());
  c->tiles_dirty = true;
  return 0;
}

// rowpart / rowbase (the two-level CDF of the detection map a data-driven birth is drawn from) and boxsum (window sums of
// the translation kernel): made when the first chain is launched
static int ensure_birth_tables(mpp_ctx *c) {
  if (c->cdf_ready) return 0;
  const size_t hw = (size_t)c->H * c->W, M = (size_t)c->n_maps;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->rowpart.alloc(M * hw)); HIPCHK(c, c->rowbase.alloc(M * (c->H + 1)));
  HIPCHK(c, c->rowtot.alloc(M * c->H)); HIPCHK(c, c->boxsum.alloc(M * hw));
  mpp_launch_cdf(c->stream, (int)M, c->det, c->H, c->W, c->rowpart, c->rowbase, c->rowtot);
  HIPCHK(c, hipGetLastError());
  c->cdf_ready = true; c->box_dirty = c->win_dirty = true; c->tiles_dirty = true;
  return 0;
}

// The birth table of a deep launch (mpp_prepass.hip), on the launch's stream right before it: every chain of the launch,
// every step it has left (at most n_steps).  pt->word stays nullptr -- the launch draws its births itself -- when the pre-pass
// is off or the table would exceed prepass_mb; pt->qoff stays nullptr -- births only -- when the queues would.
// The hot launch builds the table of the call (launch_lds): it covers every step the call has left, and the launches that
// follow with the same chain list -- the hot start's re-launch after a capacity stop, the deep launch after the handover,
// its re-launches -- read it from the step their chains have reached (PreTab::base).  A launch whose chain list differs
// (routing to device memory: compacted tile tables) builds its own.
// need_queues (the hot launch): a table without queues whose words carry positions is of no use -- nothing is launched then.
static int build_prepass(mpp_ctx *c, const DevParams *P, const TileRef *tiles, int tile0, int n, const long long *until,
                         int64_t n_steps, uint64_t seed, uint32_t chain0, PreTab *pt, bool need_queues = false) {
  *pt = PreTab{};
  if (!c->prepass || n <= 0 || n > 65535 || n_steps <= 0) return 0;       // (the chains are the grid's second dimension)
  const long long stride = n_steps;
  const int nblk = (int)((stride + PRE_BLOCK - 1) / PRE_BLOCK);
  const size_t budget = (size_t)c->prepass_mb << 20;
  const size_t cnt_off = 256, word_off = cnt_off + (((size_t)n * nblk * 4 + 255) & ~(size_t)255);
  const size_t need_b = word_off + (size_t)n * stride * 4;
  if (need_b > budget) return 0;
  // the queues (mpp_prepass.hpp): only the deep kernel of eight waves with the cost deal reads them, and only the eight kernels
  // without split / merge have one; offsets are 32-bit
  const size_t qtot_off = (need_b + 255) & ~(size_t)255, qcnt_off = qtot_off + (((size_t)n * 8 + 255) & ~(size_t)255),
               qoff_off = qcnt_off + (((size_t)n * MPP_NKERNEL * nblk * 4 + 255) & ~(size_t)255),
               qent_off = qoff_off + (((size_t)n * stride * 4 + 255) & ~(size_t)255),
               need_q = qent_off + (size_t)n * stride * sizeof(QEnt);
  const bool queues = c->prepass_queues && c->spec == 8 && (c->deep_gain & 0x100) == 0 && P->n_kernels <= MPP_K_SPLIT &&
                      stride < 0x7fffffffll && need_q <= budget;
  if (need_queues && !(queues && stride < (1ll << 28))) return 0;
  HIPCHK(c, c->pre_ws.reserve(c->stream, queues ? need_q : need_b));
  unsigned char *ws = c->pre_ws.p;
  unsigned long long *total = (unsigned long long *)ws;
  unsigned int *cnt = (unsigned int *)(ws + cnt_off);
  uint32_t *word = (uint32_t *)(ws + word_off);
  unsigned long long *qtot = queues ? (unsigned long long *)(ws + qtot_off) : nullptr;
  unsigned int *qcnt = queues ? (unsigned int *)(ws + qcnt_off) : nullptr;
  uint32_t *qoff = queues ? (uint32_t *)(ws + qoff_off) : nullptr;
  QEnt *qent = queues ? (QEnt *)(ws + qent_off) : nullptr;
  HIPCHK(c, mpp_prepass_count(c->stream, P, tiles, tile0, n, until, seed, chain0, nblk, stride, cnt, total, qcnt, qtot));
  unsigned long long births = 0;
  HIPCHK(c, hipMemcpyAsync(&births, total, sizeof births, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t rec_bytes = (size_t)births * PRE_REC_BYTES;
  // the queues and the birth records together over the budget: the births table alone may still fit (the queues' counts
  // are then left unused)
  const bool use_q = queues && need_q + rec_bytes <= budget;
  if ((use_q ? need_q : need_b) + rec_bytes > budget || (need_queues && !use_q)) return 0;
  if (!use_q) { qtot = nullptr; qcnt = nullptr; qoff = nullptr; qent = nullptr; }
  HIPCHK(c, c->pre_rec.reserve(c->stream, rec_bytes));   // (the stream is idle: synchronised just above)
  double *rec = (double *)c->pre_rec.p;
  HIPCHK(c, c->pre_base.reserve(c->stream, (size_t)n * sizeof(long long)));
  long long *base = (long long *)c->pre_base.p;
  HIPCHK(c, mpp_prepass_fill(c->stream, P, tiles, tile0, n, until, seed, chain0, nblk, stride, cnt, word, rec, qcnt, qoff, qent, base));
  pt->word = word; pt->rec = rec; pt->stride = stride; pt->base = base;
  pt->qoff = qoff; pt->qent = qent; pt->qcnt = qcnt; pt->qtot = qtot; pt->qnblk = nblk;
  return 0;
}

// One call of run_chain: its arguments, what is decided once for all its launches, the host tables they share, and the
// round of launches in hand.  decide_deep once, then per round: plan_route, launch_lds, launch_hbm, settle.
struct ChainRun {
  mpp_ctx *c;
  int grid, tile0; int64_t n_steps; uint64_t seed; uint32_t chain0;
  const mpp_proposal *d_tape; int trace_tile; mpp_step_out *d_out; mpp_proposal *d_props;
  std::vector<int32_t> herr, hn;     // per chain of the call: error word, point count, where it runs / has run, its until
  std::vector<uint8_t> in_hbm, ran_hbm;
  std::vector<long long> tab_until, h_until;
  std::vector<TileRef> tab;          // (tab, tab_until: the compacted tables of a round)
  LaunchShape sh;
  ModelClass mc;
  int deep_nmax = 0, occ = 1, hbm_waves = 8;     // deep_nmax: most steps of a deep round (0: one wave per step)
  long long trace_base = 0;
  bool hot_start = false, hot_checked = false;
  PreTab call_pt{};                  // the table the hot launch built, and the chain list it was built for
  const TileRef *call_pt_tiles = nullptr; int call_pt_tile0 = 0, call_pt_n = 0;
  bool call_pt_fits() const { return call_pt.qent && n_hbm == 0 && call_pt_tiles == tiles && call_pt_tile0 == tile0_r && call_pt_n == n_lds; }
  // this round: its LDS capacities, the chains of each home, their tile / until tables (LDS from tile0_r, the others from n_lds)
  bool decoupled;
  int lcap, lcell, n_lds, n_hbm, trace_l, trace_h, tile0_r;
  const TileRef *tiles; const long long *until;
  // the round's arguments as a launch takes them; launch_lds / launch_hbm set grid, lds, P, tile0 and trace_tile for their home
  ChainLaunch args() const {
    return ChainLaunch{c->stream, 0, 0, nullptr, tiles, 0, until, trace_base, seed, chain0, d_tape, -1, d_out, d_props};
  }
  int decide_deep(), plan_route(), launch_lds(), launch_hbm(), settle();
};

// deep rounds: chains of the shipped energy setups drawn from Philox (no tape, no split / merge, no classic image energy)
int ChainRun::decide_deep() {
  if (c->deep > 0 && c->lanes == 0 && c->spec <= 8 && !d_tape && mc.fast && !mc.split_merge &&
      (!mc.classic || c->spec == 1 || c->spec == 8) && !c->hp.force_accept && c->hp.nx < 256 && c->hp.ny < 256) {
    deep_nmax = c->deep < 64 * c->spec ? c->deep : 64 * c->spec;
    if (deep_nmax < c->spec) deep_nmax = c->spec;
    if (c->H <= 1024) c->hp.rowbase_lds = 1;
    HIPCHK(c, c->deep_stats.reserve(c->stream, 256 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->deep_stats.p, 0, 256 * sizeof(unsigned long long), c->stream));
  }
  return 0;
}

// Routing (chain_state 0, auto): a call runs every chain in LDS, exactly as without this path, until a chain no longer
// fits -- a capacity overflow that a larger LDS launch cannot hold, or a context whose capacities exceed the LDS from the
// start (where an LDS-only context stops with -12 / -11 / -7).  From then on the LDS launches keep the capacities
// that fit (lds_cap / lds_cell) and only the chains that need more -- the overflowing ones, and any whose population
// exceeds lds_cap -- go to mpp_chain_hbm_kernel, in later calls too.  An LDS launch must never see a chain with more points
// than its capacity (the kernel would clamp and write back a truncated configuration): the point counts are read back
// and each home gets a compacted tile / until table.  Its entries carry the chain's own Philox key (key_on = 1 with the
// launch's (seed, chain0 + tile) unless set by mpp_set_chain_keys), so the stream does not depend on the position.
int ChainRun::plan_route() {
  decoupled = c->lds_cap != 0;
  lcap = decoupled ? c->lds_cap : c->cap; lcell = decoupled ? c->lds_cell : c->cell_cap;
  bool route = c->chain_state == 2 || lcap < c->cap;
  for (int t = 0; t < grid && !route; ++t) route = c->hbm_tile[tile0 + t] != 0;
  n_lds = grid; n_hbm = 0;
  if (route) {
    HIPCHK(c, hipMemcpy(hn.data(), c->n + tile0, grid * sizeof(int32_t), hipMemcpyDeviceToHost));
    n_lds = 0;
    for (int t = 0; t < grid; ++t) {
      in_hbm[t] = c->chain_state == 2 || lcap < 0 || c->hbm_tile[tile0 + t] || hn[t] > lcap;
      n_lds += in_hbm[t] ? 0 : 1;
    }
    n_hbm = grid - n_lds;
  }
  trace_l = trace_tile; trace_h = -1;
  tiles = c->d_tiles; until = c->until; tile0_r = tile0;
  if (n_hbm > 0) {                       // compacted tables: LDS chains first, then the HBM chains
    if (h_until.empty()) {
      h_until.resize(grid);
      HIPCHK(c, hipMemcpy(h_until.data(), c->until + tile0, grid * sizeof(long long), hipMemcpyDeviceToHost));
    }
    HIPCHK(c, c->route.reserve(c->stream, (size_t)grid * (sizeof(TileRef) + sizeof(long long))));
    TileRef *d_route = (TileRef *)c->route.p;
    long long *d_route_until = (long long *)(d_route + grid);
    trace_l = -1;
    int il = 0, ih = n_lds;
    for (int t = 0; t < grid; ++t) {
      const int i = in_hbm[t] ? ih++ : il++;
      TileRef e = c->h_tiles[tile0 + t];
      if (!e.key_on) { e.key_on = 1; e.key_seed = seed; e.key_chain = chain0 + (uint32_t)(tile0 + t); }
      tab[i] = e; tab_until[i] = h_until[t];
      if (tile0 + t == trace_tile) (in_hbm[t] ? trace_h : trace_l) = i;
      if (in_hbm[t]) ran_hbm[t] = 1;
    }
    HIPCHK(c, hipMemcpy(d_route, tab.data(), sizeof(TileRef) * grid, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_route_until, tab_until.data(), sizeof(long long) * grid, hipMemcpyHostToDevice));
    c->hbm_chains = 0;
    for (int t = 0; t < grid; ++t) c->hbm_chains += ran_hbm[t];
    tiles = d_route; until = d_route_until; tile0_r = 0;
  }
  if (!hot_checked) {                    // (decided once per call, on the first launch's LDS chains)
    hot_start = hot_start && n_lds <= c->handover_tiles && n_lds > 0 && chain_lds_total(sh, lcap, lcell) <= MPP_LDS_LIMIT;
    hot_checked = true;
  }
  return 0;
}

// The chains whose state fits the LDS: deep rounds when they fit next to it, else one wave per step.  1: the context asks for
// more than an LDS launch holds and the capacities have just been decoupled -- plan the round again.
int ChainRun::launch_lds() {
  int rc;
  // deep rounds need room for their step reports next to the chain state: halve the round until it fits, or do without
  int nmax = deep_nmax;
  while (nmax >= sh.waves && nmax > 0 && deep_lds_total(sh, lcap, lcell, nmax) > MPP_LDS_LIMIT) nmax /= 2;
  if (nmax < sh.waves || nmax < 8) nmax = 0;
  if (lcell > 64) nmax = 0;            // (the deep kernel lists a cell's candidates in a 64-bit mask: fuller cells run one step per wave)
  if (hot_start && nmax > 0) nmax = 0;
  else hot_start = false;
  const int handover = hot_start ? c->handover_at : 0;
  if (c->hp.handover != handover) { c->hp.handover = handover; c->params_dirty = true; if ((rc = push_state(c))) return rc; }
  size_t lds = mpp_chain_lds_bytes(lcap, sh.ncell, lcell, sh.steps, sh.rb_rows, sh.waves);
  if (nmax > 0) lds = mpp_deep_lds_bytes(lcap, sh.ncell, lcell, sh.rb_rows, sh.waves, nmax, sh.ext);
  else if (chain_lds_total(sh, lcap, lcell) > MPP_LDS_LIMIT) {
    if (c->chain_state == 1)
      return fail(c, -7, "chain state needs %zu B of LDS (> %d): lower point_capacity/cell_capacity/spec_waves or tile size",
                  lds, MPP_LDS_LIMIT);
    // the context asks for more than an LDS launch holds: LDS launches keep the largest halving that fits (none: every
    // chain in device memory), the chains that do not fit it continue in device memory
    int nc = lcap, ne = lcell;
    while (nc > 64 && chain_lds_total(sh, nc, ne) > MPP_LDS_LIMIT) nc /= 2;
    while (ne > 4 && chain_lds_total(sh, nc, ne) > MPP_LDS_LIMIT) ne /= 2;
    if (chain_lds_total(sh, nc, ne) > MPP_LDS_LIMIT) nc = -1;
    c->lds_cap = nc; c->lds_cell = ne;
    return 1;
  }
  c->hp.cap = c->cap; c->hp.cell_cap = c->cell_cap;
  DevParams lp = c->hp;
  lp.cap = lcap; lp.cell_cap = lcell;
  ChainLaunch a = args();
  a.grid = n_lds; a.lds = lds; a.P = &lp; a.tile0 = tile0_r; a.trace_tile = trace_l;
  if (nmax > 0) {
    int fixed = c->deep_fixed > nmax ? nmax : c->deep_fixed;
    if (fixed > 0) { fixed = fixed / sh.waves * sh.waves; if (fixed < sh.waves) fixed = sh.waves; }
    PreTab pt{};
    if (call_pt_fits()) pt = call_pt;
    else {
      call_pt = PreTab{};                      // (a build reuses the table's buffers)
      if (!sh.ext && (rc = build_prepass(c, &lp, tiles, tile0_r, n_lds, until, n_steps, seed, chain0, &pt))) return rc;
    }
    if (pt.word) c->prepass_used = 1;
    if (pt.qoff) c->prepass_queues_used = 1;
    const int flags = (c->deep_skip_same ? MPP_DEEP_SKIP_SAME : 0) | (c->deep_carry ? MPP_DEEP_CARRY : 0);
    HIPCHK(c, mpp_launch_deep(a, sh.waves, occ, nmax, fixed, c->deep_gain, flags, (unsigned long long *)c->deep_stats.p, sh.ext, &pt));
  } else {
    // the hot start reads its steps' draws from a table (mpp_hot.hip) where the pre-pass builds one with queues whose words can
    // carry a queue position; otherwise -- and for every other one-wave-per-step launch -- the chain draws them itself
    // (MPP_NO_FAST=1 asks for the generic pair loops, mpp_sampler.hip: the table kernel has the specialised ones only)
    PreTab pt{};
    if (call_pt_fits()) pt = call_pt;
    else if (hot_start && c->hot_table && !sh.ext && !mc.no_fast) {
      if ((rc = build_prepass(c, &lp, tiles, tile0_r, n_lds, until, n_steps, seed, chain0, &pt, true))) return rc;
      call_pt = PreTab{};
      if (n_hbm == 0) { call_pt = pt; call_pt_tiles = tiles; call_pt_tile0 = tile0_r; call_pt_n = n_lds; }
    }
    if (pt.qent && pt.stride < (1ll << 28)) {
      HIPCHK(c, mpp_launch_hot(a, &pt));
      c->hot_table_used = 1;
    } else
      HIPCHK(c, mpp_launch_chain(a, c->spec, c->lanes, occ));
  }
  return 0;
}

// The chains that outgrew the LDS: state in the workspace, capacities cap / cell_cap
int ChainRun::launch_hbm() {
  const size_t stride = mpp_chain_hbm_state_bytes(c->cap, sh.ncell, c->cell_cap);
  HIPCHK(c, c->hbm_ws.reserve(c->stream, stride * (size_t)n_hbm));
  c->hp.cap = c->cap; c->hp.cell_cap = c->cell_cap;
  DevParams hpp = c->hp;
  hpp.handover = 0;
  ChainLaunch a = args();
  a.grid = n_hbm; a.lds = mpp_chain_hbm_lds_bytes(hbm_waves, sh.rb_rows); a.P = &hpp; a.tile0 = n_lds; a.trace_tile = trace_h;
  HIPCHK(c, mpp_launch_chain_hbm(a, hbm_waves, c->hbm_ws.p, stride));
  return 0;
}

// The reference's point set has no capacity (Python sets, point_set.py:45-188); a chain here lives in one workgroup's
// LDS with `point_capacity` slots and `cell_capacity` entries per cell of the spatial hash.  A step that would exceed
// either stops the chain BEFORE the step (state, temperature and step counter of that moment are written back);
// with auto_grow (default) the capacity is doubled -- as long as the chain still fits the 160 KB of LDS -- and the same
// launch is issued again: finished tiles return at once, the stopped ones continue with the very next step, so the
// chain is the one an unlimited capacity would have produced.
// settle reads the chains' error words.  0: every chain has reached its step (< 0: one stopped for good); 1: chains have
// cooled down (the hot start ends) or capacities were raised and the codes cleared: the same launch is to be issued again.
int ChainRun::settle() {
  int rc;
  HIPCHK(c, hipMemcpy(herr.data(), c->errd + tile0, grid * sizeof(int32_t), hipMemcpyDeviceToHost));
  bool cell = false, point = false, cell_h = false, point_h = false, cooled = false;
  for (int t = 0; t < grid; ++t) {
    if (herr[t] == 1) (in_hbm[t] ? cell_h : cell) = true;
    else if (herr[t] == 2) (in_hbm[t] ? point_h : point) = true;
    else if (herr[t] == 5) cooled = true;
    else if (herr[t]) return fail(c, -10 - herr[t], "tile %d: %s", tile0 + t, chain_error_text(herr[t]));
  }
  if (cooled) {                          // (a launch that ended for a capacity as well grows first and keeps its hot start)
    for (int t = 0; t < grid; ++t) if (herr[t] == 5) herr[t] = 0;
    HIPCHK(c, hipMemcpy(c->errd + tile0, herr.data(), grid * sizeof(int32_t), hipMemcpyHostToDevice));
    if (!cell && !point && !cell_h && !point_h) { hot_start = false; return 1; }
  }
  if (!cell && !point && !cell_h && !point_h) return 0;
  // the first stopped chain, and why it cannot go on
  auto stop = [&](const char *why) {
    for (int t = 0; t < grid; ++t)
      if (herr[t]) return fail(c, -10 - herr[t], "tile %d: %s (%s)", tile0 + t, chain_error_text(herr[t]), why);
    return fail(c, -1, "no stopped chain");
  };
  if (!c->auto_grow) return stop("auto_grow is off");
  int new_cap = c->cap, new_cell = c->cell_cap;
  if (cell || point) {                     // LDS chains: double the LDS launch's capacity where that still fits the LDS
    int nl_cap = lcap, nl_cell = lcell;
    bool r_cell = false, r_point = false;  // ... and where it does not, those chains continue in device memory
    if (cell) {
      const int v = doubled(lcell, MPP_CELL_CAP_MAX);
      if (v == lcell) return stop("cell_capacity is at its limit");
      if (chain_lds_total(sh, nl_cap, v) <= MPP_LDS_LIMIT) nl_cell = v; else r_cell = true;
    }
    if (point) {
      const int v = doubled(lcap, 65535);
      if (v == lcap) return stop("point_capacity is at its limit 65535 (16-bit slot indices)");
      if (chain_lds_total(sh, v, nl_cell) <= MPP_LDS_LIMIT) nl_cap = v; else r_point = true;
    }
    if ((r_cell || r_point) && c->chain_state == 1)
      return stop("larger capacities do not fit the chain's LDS budget and chain_state is 1: LDS only");
    if (r_cell || r_point) {
      if (!decoupled) { c->lds_cap = lcap; c->lds_cell = lcell; }
      for (int t = 0; t < grid; ++t)
        if (!in_hbm[t] && ((herr[t] == 1 && r_cell) || (herr[t] == 2 && r_point))) c->hbm_tile[tile0 + t] = 1;
      if (r_cell && doubled(lcell, MPP_CELL_CAP_MAX) > new_cell) new_cell = doubled(lcell, MPP_CELL_CAP_MAX);
      if (r_point && doubled(lcap, 65535) > new_cap) new_cap = doubled(lcap, 65535);
    }
    if (c->lds_cap != 0) { c->lds_cap = nl_cap; c->lds_cell = nl_cell; }
    if (nl_cap > new_cap) new_cap = nl_cap;
    if (nl_cell > new_cell) new_cell = nl_cell;
  }
  if (point_h) {
    if (c->cap >= 65535) return stop("point_capacity is at its limit 65535 (16-bit slot indices)");
    if (doubled(c->cap, 65535) > new_cap) new_cap = doubled(c->cap, 65535);
  }
  if (cell_h) {
    if (c->cell_cap >= MPP_CELL_CAP_MAX) return stop("cell_capacity is at its limit");
    if (doubled(c->cell_cap, MPP_CELL_CAP_MAX) > new_cell) new_cell = doubled(c->cell_cap, MPP_CELL_CAP_MAX);
  }
  if (new_cap > c->cap && (rc = grow_points(c, new_cap))) return rc;
  c->cell_cap = new_cell; c->grow_events += 1;
  // clear the two overflow codes (sticky otherwise) and bring the tile table / parameters up to date
  for (int t = 0; t < grid; ++t) if (herr[t] == 1 || herr[t] == 2) herr[t] = 0;
  HIPCHK(c, hipMemcpy(c->errd + tile0, herr.data(), grid * sizeof(int32_t), hipMemcpyHostToDevice));
  c->params_dirty = true;
  if ((rc = push_state(c))) return rc;
  return 1;
}

static int run_chain(mpp_ctx *c, int grid, int tile0, int64_t n_steps, uint64_t seed, uint32_t chain0,
                     const mpp_proposal *d_tape, int trace_tile, mpp_step_out *d_out, mpp_proposal *d_props) {
  if (!c->have_kernels) return fail(c, -1, "mpp_set_kernels has not been called");
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  if (!c->have_model) return fail(c, -1, "mpp_set_model has not been called");
  int rc;
  if ((rc = ensure_birth_tables(c)) || (rc = ensure_remap_tables(c)) || (rc = push_state(c))) return rc;
  // the row level of the birth CDF goes to LDS when it fits and the chain speculates (it shortens the slowest
  // wave of a round); throughput launches of one-wave chains keep their LDS for occupancy
  c->hp.rowbase_lds = (c->H <= 1024 && (c->lanes > 0 || c->spec > 1)) ? 1 : 0;
  const ModelClass mc = model_class(c->hp);
  if (mc.extended() && !(c->lanes == 0 && (c->spec == 1 || c->spec == 8)))
    return fail(c, -1, "the split / merge kernels and the classic image energies are built for spec_waves 1 or 8 with spec_lanes 0");
  ChainRun k{c, grid, tile0, n_steps, seed, chain0, d_tape, trace_tile, d_out, d_props, std::vector<int32_t>(grid), std::vector<int32_t>(grid),
             std::vector<uint8_t>(grid, 0), std::vector<uint8_t>(grid, 0), std::vector<long long>(grid), {}, std::vector<TileRef>(grid)};
  k.mc = mc;
  if ((rc = k.decide_deep())) return rc;
  k.sh = launch_shape(c, c->hp.rowbase_lds != 0);
  mpp_launch_set_until(c->stream, c->d_tiles, tile0, grid, (long long)n_steps, c->until);
  HIPCHK(c, hipGetLastError());
  if (trace_tile >= 0) {
    int64_t s0 = 0;
    HIPCHK(c, hipMemcpyAsync(&s0, c->step + trace_tile, sizeof s0, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    k.trace_base = s0;
  }
  c->last_ms = 0.0;
  c->hbm_chains = 0; c->prepass_used = 0; c->prepass_queues_used = 0; c->hot_table_used = 0;
  if ((int)c->hbm_tile.size() != c->n_tiles) c->hbm_tile.assign(c->n_tiles, 0);
  k.occ = (grid >= 1024) ? 2 : 1;          // many chains in one launch: prefer the instantiation that lets two waves share a SIMD
  k.hbm_waves = (c->lanes == 0 && c->spec == 1) ? 1 : 8;
  // hot start: one wave per step until the chain has cooled down (ERR_HANDOVER), then deep rounds -- the same chain either way
  // (launches of a few chains only: the launch that hands over ends when its LAST chain has cooled down, the others' CUs idle
  //  until then -- 256 tiles of config 5's scene lost 3 ms to that, one tile gains 6)
  k.hot_start = k.deep_nmax > 0 && c->handover && c->spec == 8 && c->lanes == 0 && trace_tile < 0 && !c->deep_fixed && n_steps >= 4096;
  // plan the routing, launch the chains of either home, read the error words; again while chains cool down or grow
  for (;;) {
    if ((rc = k.plan_route())) return rc;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (k.n_lds > 0 && (rc = k.launch_lds())) { if (rc == 1) continue; return rc; }
    if (k.n_hbm > 0 && (rc = k.launch_hbm())) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_ms += ms;
    if ((rc = k.settle()) <= 0) return rc;
  }
}

extern "C" int mpp_replay(mpp_ctx *c, int tile, int n, const mpp_proposal *tape, mpp_step_out *out) {
  int rc = check_tile(c, tile);
  if (rc) return rc;
  if (n <= 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<mpp_proposal> d_tape;
  DevBuf<mpp_step_out> d_out;
  HIPCHK(c, d_tape.alloc((size_t)n));
  if (out) HIPCHK(c, d_out.alloc((size_t)n));
  hipError_t e = hipMemcpyAsync(d_tape, tape, (size_t)n * sizeof(mpp_proposal), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) rc = run_chain(c, 1, tile, n, 0, 0, d_tape, tile, d_out, nullptr);
  if (e == hipSuccess && out)
    e = hipMemcpy(out, d_out, (size_t)n * sizeof(mpp_step_out), hipMemcpyDeviceToHost);
  HIPCHK(c, e);
  return rc;
}

extern "C" int mpp_run(mpp_ctx *c, int64_t n_steps, uint64_t seed, uint32_t chain0, int trace_tile, mpp_step_out *out,
                       mpp_proposal *props) {
  if (!c) return -1;
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  if (n_steps <= 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<mpp_step_out> d_out;
  DevBuf<mpp_proposal> d_props;
  bool tr = trace_tile >= 0 && trace_tile < c->n_tiles;
  if (tr && out) HIPCHK(c, d_out.alloc((size_t)n_steps));
  if (tr && props) HIPCHK(c, d_props.alloc((size_t)n_steps));
  int rc = run_chain(c, c->n_tiles, 0, n_steps, seed, chain0, nullptr, tr ? trace_tile : -1, d_out, d_props);
  hipError_t e = hipSuccess;
  if (d_out) e = hipMemcpy(out, d_out, (size_t)n_steps * sizeof(mpp_step_out), hipMemcpyDeviceToHost);
  if (d_props && e == hipSuccess) e = hipMemcpy(props, d_props, (size_t)n_steps * sizeof(mpp_proposal), hipMemcpyDeviceToHost);
  HIPCHK(c, e);
  return rc;
}

// ---- parallel tempering (mpp_tempering.hip) -----------------------------------------------------
extern "C" int mpp_get_schedules(mpp_ctx *c, double *sched) {
  if (!c || !sched) return fail(c, -1, "bad get_schedules arguments");
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(sched, c->T, (size_t)c->n_tiles * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
extern "C" int mpp_set_schedules(mpp_ctx *c, const double *sched) {
  if (!c || !sched) return fail(c, -1, "bad set_schedules arguments");
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  for (int t = 0; t < c->n_tiles; ++t) {
    const double *s = sched + 3 * (size_t)t;
    if (!std::isfinite(s[0]) || !std::isfinite(s[1]) || !std::isfinite(s[2]))
      return fail(c, -1, "set_schedules: chain %d has an entry that is not finite", t);
    if (s[0] < s[2]) return fail(c, -1, "set_schedules: chain %d has T < T_target", t);
  }
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(c->T, sched, (size_t)c->n_tiles * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int mpp_set_ladder(mpp_ctx *c, double ratio) {
  if (!c) return -1;
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  const int R = c->replicas, n = c->n_maps, T = c->n_tiles;
  if (R < 2) return fail(c, -1, "set_ladder: a ladder needs replicas >= 2, the ctx holds %d", R);
  if (!std::isfinite(ratio) || !(ratio >= 1.0)) return fail(c, -1, "set_ladder: ratio must be finite and >= 1");
  std::vector<double> sched((size_t)T * 3);
  std::vector<int32_t> rung(T);
  double f = 1.0;
  for (int r = 0; r < R; ++r) {
    if (r > 0) f *= ratio;
    if (!std::isfinite(c->sched[0] * f)) return fail(c, -1, "set_ladder: the temperature of rung %d is not finite", r);
    for (int i = 0; i < n; ++i) {
      double *s = sched.data() + 3 * ((size_t)r * n + i);
      s[0] = c->sched[0] * f; s[1] = c->sched[1]; s[2] = c->sched[2] * f;
      rung[(size_t)r * n + i] = r;
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->rung.p) HIPCHK(c, c->rung.alloc((size_t)T));
  if (!c->x_acc.p) HIPCHK(c, c->x_acc.alloc((size_t)n * (R - 1)));
  HIPCHK(c, hipMemcpyAsync(c->T, sched.data(), sched.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->rung, rung.data(), (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->x_acc, 0, (size_t)n * (R - 1) * sizeof(long long), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->ladder = true;
  c->x_exchanges = c->x_attempts = 0; c->x_ms = 0.0;
  return 0;
}

extern "C" int mpp_run_tempered(mpp_ctx *c, int64_t n_steps, uint64_t seed, uint32_t chain0, int64_t every,
                                mpp_exchange_record *log, int64_t log_cap, int64_t *n_logged) {
  if (!c) return -1;
  if (n_logged) *n_logged = 0;
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  if (!c->ladder || !c->rung.p) return fail(c, -1, "run_tempered: no ladder is set (mpp_set_ladder)");
  if (every < 1) return fail(c, -1, "run_tempered: every must be >= 1");
  if (log && log_cap < 0) return fail(c, -1, "run_tempered: log_cap must be >= 0");
  if (n_steps <= 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  const int T = c->n_tiles, R = c->replicas, n = c->n_maps;
  std::vector<int64_t> step(T);
  HIPCHK(c, hipMemcpyAsync(step.data(), c->step, (size_t)T * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int t = 1; t < T; ++t)
    if (step[t] != step[0])
      return fail(c, -1, "run_tempered: chain %d is at step %lld, chain 0 at %lld: an exchange needs all chains at the same step", t,
                  (long long)step[t], (long long)step[0]);
  const int64_t s0 = step[0], s1 = s0 + n_steps;
  // pairs of exchange e (mpp_launch_exchange): the records of the call are numbered ahead, exchange by exchange
  auto pairs = [R](int64_t e) { return (int64_t)((R - (R == 2 ? 0 : (int)(e & 1))) / 2); };
  int64_t total = 0;
  for (int64_t s = (s0 / every + 1) * every; s <= s1; s += every) total += (int64_t)n * pairs(s / every);
  if (!log) log_cap = 0;
  const int64_t kept = total < log_cap ? total : log_cap;
  if (kept > 0 && c->x_log.reserve(c->stream, (size_t)kept * sizeof(mpp_exchange_record)) != hipSuccess)
    return fail(c, -2, "no device memory for %lld exchange records", (long long)kept);
  mpp_exchange_record *d_log = kept > 0 ? (mpp_exchange_record *)c->x_log.p : nullptr;
  double ms_sum = 0.0;
  int hbm = 0, pre = 0, que = 0, hot = 0;
  bool timing = false;                         // ev2 / ev3 hold an exchange whose time has not been read
  auto take_time = [&]() {                     // (after a wait for the stream)
    float ms = 0.f;
    if (timing && hipEventElapsedTime(&ms, c->ev2, c->ev3) == hipSuccess) c->x_ms += ms;
    timing = false;
  };
  int64_t base = 0;
  int rc = 0;
  for (int64_t pos = s0; pos < s1;) {
    const int64_t next = (pos / every + 1) * every, to = next < s1 ? next : s1;
    rc = run_chain(c, T, 0, to - pos, seed, chain0, nullptr, -1, nullptr, nullptr);   // (it ends with the stream idle)
    ms_sum += c->last_ms;
    hbm = c->hbm_chains > hbm ? c->hbm_chains : hbm;
    pre |= c->prepass_used; que |= c->prepass_queues_used; hot |= c->hot_table_used;
    take_time();
    if (rc) break;
    pos = to;
    if (pos % every) continue;
    double *d_e = nullptr;
    if ((rc = push_state(c))) break;
    HIPCHK(c, hipEventRecord(c->ev2, c->stream));
    if ((rc = chain_energy_launches(c, &d_e))) break;
    mpp_launch_exchange(c->stream, c->d_tiles, n, R, c->T, c->rung, d_e, (long long)pos, (long long)(pos / every), seed, chain0,
                        c->x_acc, d_log, (long long)base, (long long)kept);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev3, c->stream));
    timing = true;
    base += (int64_t)n * pairs(pos / every);
    c->x_exchanges += 1; c->x_attempts += (int64_t)n * pairs(pos / every);
  }
  c->last_ms = ms_sum;
  c->hbm_chains = hbm; c->prepass_used = pre; c->prepass_queues_used = que; c->hot_table_used = hot;
  hipError_t e = hipSuccess;
  if (rc == 0 && kept > 0) e = hipMemcpyAsync(log, d_log, (size_t)kept * sizeof(mpp_exchange_record), hipMemcpyDeviceToHost, c->stream);
  hipError_t e2 = hipStreamSynchronize(c->stream);
  take_time();
  if (rc) return rc;
  HIPCHK(c, e); HIPCHK(c, e2);
  if (n_logged) *n_logged = base;
  return 0;
}

extern "C" int mpp_step_index(mpp_ctx *c, int tile, int64_t *step) {
  int rc = check_tile(c, tile);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy(step, c->step + tile, sizeof(int64_t), hipMemcpyDeviceToHost));
  return 0;
}
extern "C" int mpp_last_kernel_ms(mpp_ctx *c, double *ms) {
  if (!c || !ms) return -1;
  *ms = c->last_ms;
  return 0;
}
