// mpp_ctx.hpp -- the context behind the C ABI of include/mpp_hip.h, shared by the host-API files (mpp_api*.hip): the two
// types that own its device memory, struct mpp_ctx, the error helpers, and the launch shape of a chain.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "mpp_launch.hpp"
#include "mpp_detect.hpp"
#include "mpp_train.hpp"
#include "mpp_rescale.hpp"

#define MPP_CELL_CAP_MAX 2048    // entries of a 32-px cell of the spatial hash (16-bit counts); what fits the LDS decides

// A device array freed with its owner: a call's temporaries (on every way out of the call) and the arrays the context
// keeps.  alloc() drops what it held and takes room for `count` elements, at least one.
template <typename T>
struct DevBuf {
  T *p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf &&o) : p(o.p) { o.p = nullptr; }
  DevBuf &operator=(DevBuf &&o) { std::swap(p, o.p); return *this; }
  ~DevBuf() { reset(); }
  void reset() { if (p) (void)hipFree(p); p = nullptr; }
  hipError_t alloc(size_t count) { reset(); return hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)); }
  operator T *() const { return p; }
};
// A workspace that only grows: reserve() keeps a block that is large enough, and waits for the stream before it frees a
// live one (launches on it may still read the block).
struct DevWs : DevBuf<unsigned char> {
  size_t bytes = 0;
  hipError_t reserve(hipStream_t st, size_t need) {
    if (need <= bytes) return hipSuccess;
    hipError_t e = p ? hipStreamSynchronize(st) : hipSuccess;
    if (e != hipSuccess) return e;
    bytes = 0;
    if ((e = alloc(need)) == hipSuccess) bytes = need;
    return e;
  }
};

// the device arrays sized by mpp_set_maps: dropped together when the maps are replaced
struct TileMem {
  DevBuf<double> rowpart, rowbase, rowtot, boxsum, rowwin, ps, pr, pa, T;
  DevBuf<int32_t> px, py, n, errd;
  DevBuf<int64_t> step;
  DevBuf<long long> until;           // per tile: the absolute step the current mpp_run / mpp_replay call runs it to
  DevBuf<double> remap[3];           // tables of the remapped marks (chains only), see ensure_remap_tables
  DevBuf<TileRef> d_tiles;
  DevBuf<int32_t> rung;              // parallel tempering (mpp_set_ladder): per chain, its place on its tile's temperature ladder
  DevBuf<long long> x_acc;           // ... and per (tile, pair of neighbouring rungs) the accepted exchanges
};

struct mpp_ctx : TileMem {
  int device = 0;
  hipStream_t stream = nullptr, own_stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev2 = nullptr, ev3 = nullptr;     // around the energy and exchange launches of mpp_run_tempered
  std::string err;
  DevParams hp;
  DevBuf<DevParams> dp;
  bool params_dirty = true, tiles_dirty = true, have_model = false, have_kernels = false, have_maps = false;
  int n_tiles = 0, H = 0, W = 0;
  bool maps_borrowed = false;
  float *det = nullptr, *m[3] = {nullptr, nullptr, nullptr};
  float *img = nullptr;              // the picture behind the classic image energies (mpp_set_image), [n_maps][H][W][img_c]
  int img_c = 0;
  bool img_borrowed = false;
  bool box_dirty = true;
  bool cdf_ready = false;          // rowpart / rowbase / boxsum exist (made by the first launch that draws births)
  // the data-driven translation reads its window's row sums from the transposed table rowwin (mpp_window.hpp; option
  // window_rows, 0: the chains get a null pointer and form the sums from rowpart).  The table is made with boxsum, from the
  // first push_state that finds the option on; win_dirty: it is not the one of the current maps and max_delta
  int window_rows = 1;
  bool win_dirty = true;
  int cap = 1024, cell_cap = 32, spec = 1, lanes = 0;
  // deep rounds (mpp_deep.hip): every lane of the chain's `spec` waves evaluates one step, at most `deep` steps per round
  // (default 128; 0 = off: one wave per step); deep_fixed > 0 pins the number of steps per round (tests); deep_stats: rounds, evaluated
  // steps, rounds with a change, committed steps of the last mpp_run (device counters, read on request)
  int handover = 1;                  // start a chain of 8 waves with one wave per step and hand it to the deep rounds once it has cooled down
  int handover_at = 1280;            // ... when the smoothed steps committed per round of 8 reach this / 256 (5.0: one tile is flat from 4.5 to 6.5, 64 tiles want it early -- 34.8 ms at 5.0, 36.3 at 5.5, 42 at 6.5)
  int handover_tiles = 64;           // ... in launches of at most this many chains (64 tiles of config 4: -6 %; 256 of config 5: +4 %)
  int deep = 128, deep_fixed = 0, deep_gain = 12;   // deep_gain / 8 x the steps the last rounds committed = depth of the next (12: 4 % faster than 16 on the bench tile and on config 5's chains, 10 and 20 slower)
  // deep_skip_same 1: an untraced deep round does not evaluate a move / transform that proposes the values its target already
  // holds (the step changes nothing, accepted or not, and nothing reads its outcome); 0: every step is evaluated.  It travels
  // as a flag of mpp_launch_deep, not in DevParams: the block is an argument of every chain kernel, and a field more
  // would move the arguments behind it in kernels this option has nothing to do with
  int deep_skip_same = 1;
  // deep_carry 1: a queue round keeps the non-changing reports behind its end that no change it committed conflicts with
  // (carry_keeps, mpp_commit.hpp), and the next round does not evaluate their steps again; 0: every step of a window is
  // evaluated.  A flag of mpp_launch_deep like deep_skip_same, for the same reason
  int deep_carry = 1;
  DevWs deep_stats;
  // the birth pre-pass of a deep launch (mpp_prepass.hip): prepass 1 on, 0 off (the chains draw their births themselves);
  // a launch whose table would exceed prepass_mb MB runs without one; prepass_used: a deep launch of the last call used one
  int prepass = 1, prepass_mb = 256, prepass_used = 0;
  // ... and with it the steps of every kernel type in queues (prepass_queues 1), from which the rounds of a chain of eight
  // waves take their steps (the deep kernel's QUE instantiation); prepass_queues_used: a deep launch of the last call did
  int prepass_queues = 1, prepass_queues_used = 0;
  // ... and the hot start takes its steps' draws from a table of its own launch (hot_table 1: mpp_hot.hip; it needs the queues);
  // hot_table_used: a hot launch of the last call read one
  int hot_table = 1, hot_table_used = 0;
  DevWs pre_ws;                      // the table's total, block counts and step words
  DevWs pre_rec;                     // its birth records
  DevWs pre_base;                    // per chain of the table: the step its part starts at (PreTab::base)
  int replicas = 1, n_maps = 0;      // n_tiles = n_maps * replicas chains; chain t samples on the maps of tile t % n_maps
  bool remap_dirty = true;
  int remap_mode = -1;               // option "remap_table": -1 auto (when the tables fit remap_budget), 0 never, 1 always
  // 2 GB: a handful of tiles sampled for many steps (BASELINE configs 2 and 3: 0.2 GB per 512-px tile).  With the 256 tiles
  // of a 4096-px image the tables would be 12.9 GB: 3.7 ms less kernel time (5 %) for >= 6 ms of building them and a 13 GB
  // hipMalloc whose cost varies between 0 and 1.4 s (profiles/tools/probe_remap_cost.py) -- not worth it.
  size_t remap_budget = (size_t)2 << 30;
  int auto_grow = 1, grow_events = 0; // capacity overflow -> raise the capacity and continue (see run_chain)
  // Where a chain's state lives (option chain_state, see run_chain): 0 auto, 1 LDS only, 2 device memory for every chain.
  // cap / cell_cap are the context's capacities (cap is also the stride of the configuration arrays); an LDS launch runs
  // with lds_cap / lds_cell once the two have been decoupled (0: the same as cap / cell_cap; lds_cap -1: no LDS launch fits)
  int chain_state = 0;
  int lds_cap = 0, lds_cell = 0;
  std::vector<uint8_t> hbm_tile;     // per chain: an LDS launch could not hold it, it continues in device memory
  int hbm_chains = 0;                // chains that ran at least one launch in device memory in the last mpp_run / mpp_replay
  DevWs hbm_ws;                      // their workspace (contents rebuilt by every launch)
  DevWs route;                       // per-launch tile table, then until table, of a call whose chains are split between the two homes
  std::vector<double> intensity;
  std::vector<uint64_t> key_seed;    // per-chain Philox key / chain id (mpp_set_chain_keys); empty: the launch's seed, chain0 + tile
  std::vector<uint32_t> key_chain;
  std::vector<TileRef> h_tiles;
  double sched[3] = {1.0, 1.0, 0.0};
  double last_ms = 0.0;
  // parallel tempering: a ladder is set (rung / x_acc exist); exchange steps and attempted pairs since then, the time of their
  // launches; the device log of the call in hand
  bool ladder = false;
  int64_t x_exchanges = 0, x_attempts = 0;
  double x_ms = 0.0;
  DevWs x_log;
  // uniform grid over one tile's configuration for the from-scratch energies (built per call; see mpp_scratch.hip).  It stays
  // apart from grids_ws: its threshold is the tile's actual count, not the capacity
  DevWs g_cells, g_items;            // cell starts [ncell + 1] then cursors [ncell]; the points by cell [cap]
  int grid_min_points = 256;
  DevWs grids_ws;                    // the candidate grids of every chain (chain_grids_build): rebuilt right before their one consumer
  DevWs energy_ws;                   // mpp_total_energy_all: every chain's point energies, their sums
  DevWs birth_ws;                    // mpp_birth_energy_map: the per-point cache, the summary's parts
  int birth_grid = 0;                // ... its last pre-pass built candidate grids
  DevWs minsel_ws;                   // mpp_select_minima / mpp_birth_complete / mpp_descend: the candidate list and its tables
  DevWs recombine_ws;                // mpp_recombine: the tiles' labels and cluster choices, the staged composites, the reports
  DevWs descent_ws;                  // mpp_descend / mpp_birth_complete / mpp_papangelou_all: the Papangelou values, the maps, the round's lists, the reports
  DevWs ptsel_ws;                    // mpp_select_points: its two counters
  DevWs relocate_ws;                 // mpp_move_gains / mpp_relocate: the per-point cache, the target pixels, the books
  int move_grid = 0;                 // ... its last pre-pass built candidate grids
  int recombine_lds = MPP_RECOMBINE_LDS_POINTS;   // ... a tile of more points over its replicas labels in the workspace, not in LDS
  DetectWs detect;                   // workspace of mpp_detect_centers (mpp_detect.hip)
  TrainWs train;                     // workspace of the loss kernels (mpp_train.hip)
  RescaleWs rescale;                 // workspace of mpp_rescale (mpp_rescale.hip)
  DevWs figures;                     // workspace of mpp_draw_outlines (mpp_figures.hip): the tables, then the owner image
};

static int fail(mpp_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}
#define HIPCHK(c, call)                                                                            \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) return fail(c, -2, "%s failed: %s", #call, hipGetErrorString(e_));       \
  } while (0)

int push_state(mpp_ctx *c);             // (mpp_api.hip)
int check_tile(mpp_ctx *c, int tile);

// The candidate grids of every chain (mpp_launch_grid_build_all): start [T][ncell + 1], cursor [T][ncell], items [T][cap] in
// grids_ws.  Off: null pointers and ncell 0, and the kernels scan the whole configuration.
struct ChainGrids {
  int32_t *start = nullptr, *cursor = nullptr, *items = nullptr;
  int ncell = 0;
};
// The passes over every chain keep the counts on the device, so their grids are on whenever a chain could reach
// scratch_grid_min_points (mpp_merge_score, which knows the counts, has a rule of its own).
static bool chain_grids_on(const mpp_ctx *c) {
  return c->grid_min_points > 0 && c->hp.nx * c->hp.ny > 0 && c->cap >= c->grid_min_points;
}
// When `on`, build the grids over the first max_n slots of every chain; nonzero: no device memory.  They serve the launches
// that follow on the context's stream up to the next build, and *g holds for that long only: reserve may move the block.
static int chain_grids_build(mpp_ctx *c, int max_n, bool on, ChainGrids *g) {
  *g = ChainGrids{};
  if (!on) return 0;
  const int ncell = c->hp.nx * c->hp.ny;
  const size_t T = (size_t)c->n_tiles;
  if (c->grids_ws.reserve(c->stream, T * (2 * (size_t)ncell + 1 + c->cap) * sizeof(int32_t)) != hipSuccess) return -2;
  g->start = (int32_t *)c->grids_ws.p; g->cursor = g->start + T * (ncell + 1); g->items = g->cursor + T * ncell;
  g->ncell = ncell;
  mpp_launch_grid_build_all(c->stream, c->dp, c->d_tiles, c->n_tiles, max_n, ncell, c->cap, g->start, g->cursor, g->items);
  return 0;
}

// The launches of mpp_total_energy_all, after push_state: every chain's energy, from the written-back state, stays on the
// device in *d_sum [n_chains] (workspace energy_ws).  The point energies of all chains in one launch (the kernel of
// mpp_total_energy, so the same bits), their sums in slot order.  Each chain uses its grid only from scratch_grid_min_points
// points on.
static int chain_energy_launches(mpp_ctx *c, double **d_sum) {
  const int T = c->n_tiles;
  if (T > 65535) return fail(c, -1, "total_energy_all: %d chains, at most 65535", T);
  const size_t TC = (size_t)T * c->cap;
  ChainGrids g;
  if (c->energy_ws.reserve(c->stream, (TC + (size_t)T) * sizeof(double)) != hipSuccess ||
      chain_grids_build(c, c->cap, chain_grids_on(c), &g))
    return fail(c, -2, "no device memory for the energies of %d chains", T);
  double *e_pts = (double *)c->energy_ws.p;
  *d_sum = e_pts + TC;
  mpp_launch_chain_energies(c->stream, c->dp, c->d_tiles, T, c->cap, e_pts, *d_sum, g.start, g.items, g.ncell + 1, c->grid_min_points);
  HIPCHK(c, hipGetLastError());
  return 0;
}

static const char *chain_error_text(int e) {
  static const char *const text[] = {"a cell of the spatial hash holds more points than cell_capacity allows",
                                     "point capacity of the tile exceeded",
                                     "proposal refers to a point that does not exist or lies outside the tile",
                                     "candidate list overflow (lower cell_capacity or report)"};
  return e >= 1 && e <= 4 ? text[e - 1] : "unknown chain error";
}

// What the launches of a chain have in common, taken once from the context.
struct LaunchShape {
  int waves;       // waves of a chain's workgroup (lane mode: 4)
  int steps;       // steps it evaluates per round, one wave (or lane group) each
  int ncell;       // cells of the spatial hash
  int rb_rows;     // rows of the birth CDF's row level that are copied to LDS (0: read from device memory)
  int ext;         // the model has a classic image energy
};
static LaunchShape launch_shape(const mpp_ctx *c, bool rowbase_lds) {
  return LaunchShape{c->lanes > 0 ? 4 : c->spec, c->lanes > 0 ? 4 * c->lanes : c->spec, c->hp.nx * c->hp.ny,
                     rowbase_lds ? c->H + 1 : 0, model_class(c->hp).classic ? 1 : 0};
}
// dynamic + static LDS of a chain with one wave per step / in deep rounds of at most nmax steps: what has to fit a CU's 160 KB
static size_t chain_lds_total(const LaunchShape &s, int cap, int cell_cap) {
  return mpp_chain_lds_bytes(cap, s.ncell, cell_cap, s.steps, s.rb_rows, s.waves) + mpp_chain_static_lds_bytes(s.waves);
}
static size_t deep_lds_total(const LaunchShape &s, int cap, int cell_cap, int nmax) {
  return mpp_deep_lds_bytes(cap, s.ncell, cell_cap, s.rb_rows, s.waves, nmax, s.ext) + mpp_chain_static_lds_bytes(s.waves);
}
static int doubled(int v, int limit) { return v * 2 > limit ? limit : v * 2; }
