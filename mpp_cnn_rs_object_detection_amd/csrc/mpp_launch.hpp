// mpp_launch.hpp -- the host launchers and LDS-size functions of the kernel files, declared once and included by the file that
// defines each and by the API files that call them: extern "C" symbols link whatever their prototype says, here a drift fails to compile.
#pragma once
#include <cstddef>
#include <cstdlib>

#include "mpp_device.hpp"
#include "mpp_prepass.hpp"

#define MPP_LDS_LIMIT (160 * 1024)                 // the LDS of a CU: what a chain's dynamic + static LDS has to fit
#define MPP_DEDUPE_LDS_MAX (MPP_LDS_LIMIT - 256)   // the most the dedupe walk of mpp_merge_score may ask for (k_dedupe_tiles)

// What every chain launch is given: ChainRun (mpp_api_chain.hip) fills one per round, the launchers pass it down to the
// hipLaunchKernelGGL of the instantiation they pick, where the kernel takes the fields as its individual arguments.
struct ChainLaunch {
  hipStream_t st; int grid; size_t lds;          // the chains are tiles[tile0 .. tile0 + grid); lds: the kernel's dynamic LDS
  const DevParams *P;                            // (host) the parameter block, passed by value
  const TileRef *tiles; int tile0; const long long *until;
  long long trace_base; unsigned long long seed; unsigned int chain0;
  const mpp_proposal *tape;                      // replay: the proposals to take instead of Philox draws
  int trace_tile; mpp_step_out *out; mpp_proposal *props;   // the tile whose steps are recorded (-1: none), and where
};

// Which kind of model runs: it decides the instantiation a launch takes and what run_chain may do with the chains.
struct ModelClass {
  bool fast;         // pair 0 = rectangle overlap / max, pair 1 = alignment / min -- both shipped setups: the FAST pair loops apply
  bool classic;      // a classic image energy among the unit terms (energies/classics.py) ...
  bool gradient;     // ... the gradient one among them
  bool split_merge;  // split / merge kernels in the mixture
  bool no_fast;      // MPP_NO_FAST=1: the launches that have the choice keep the generic pair loops
  bool extended() const { return classic || split_merge; }   // the SM / EXT instantiations, built for 1 and 8 waves
};
static inline ModelClass model_class(const DevParams &P) {
  static const bool no_fast = getenv("MPP_NO_FAST") != nullptr;
  const mpp_model &M = P.model;
  ModelClass m{};
  m.fast = M.n_pair == 2 && M.pair[0].kind == MPP_P_OVERLAP && M.pair[0].reduce == MPP_REDUCE_MAX &&
           M.pair[1].kind == MPP_P_ALIGN && M.pair[1].reduce == MPP_REDUCE_MIN;
  for (int k = 0; k < M.n_unit; ++k) {
    m.classic = m.classic || M.unit[k].kind == MPP_U_CONTRAST || M.unit[k].kind == MPP_U_GRADIENT;
    m.gradient = m.gradient || M.unit[k].kind == MPP_U_GRADIENT;
  }
  m.split_merge = P.n_kernels > MPP_K_SPLIT;
  m.no_fast = no_fast;
  return m;
}

// What the pre-pass of the birth-energy map keeps per point of a chain, [n_chains][cap] each: the unit part of its energy,
// its gate, its two pair reductions and its energy in the chain's configuration.
struct BirthCache { double *lin, *r0, *r1, *e; int32_t *gate; };
#define MPP_BIRTH_PARTS 256                        // partial summaries per chain (one per workgroup of the first pass)
struct BirthPart { double v; long long idx, n_neg, n_nan; };   // smallest non-NaN value and its row-major index (-1: none)

// One selection of local minima over the maps of n_chains chains (mpp_birth_complete.hip), all device.  The caller sets the
// first block; mpp_minsel_plan places the arrays of the second in a workspace of mpp_minsel_bytes bytes.
struct MinSel {
  const double *dE; size_t chain_stride;           // chain t's map starts at dE + t * chain_stride, rows ld apart
  int H, W, ld, n_chains;
  double below, d2;                                // candidates: dE < below; within reach: (double)(dx*dx + dy*dy) <= d2
  int reach;                                       // no pixel further than this in a row or a column is within reach
  const mpp_descent_report *rep;                   // nullptr, or [n_chains]: a chain whose status is >= 0 has no candidates
  int nb_fill, nb_res;                             // blocks per chain of the compaction and of the resolve
  double *val; int32_t *idx;                       // the candidates in row-major order, [n_chains][H*W]
  int32_t *rows;                                   // [n_chains][H+1]: where a row's candidates start in the list
  int32_t *cblk, *kblk;                            // per block: candidates / kept candidates in front of it
  int32_t *n_cand, *n_kept;                        // [n_chains]
  uint8_t *keep;                                   // [n_chains][H*W], by place in the list
};

// flags of mpp_launch_deep
#define MPP_DEEP_SKIP_SAME 1                       // option deep_skip_same: steps that re-write their target unchanged are not evaluated
#define MPP_DEEP_CARRY 2                           // option deep_carry: the queue rounds keep the reports no commit of the round touched

extern "C" {
size_t mpp_chain_lds_bytes(int cap, int ncell, int cell_cap, int spec, int rowbase_n, int waves);
size_t mpp_chain_static_lds_bytes(int waves);      // the staged parameter block: the same for every chain kernel
size_t mpp_chain_hbm_state_bytes(int cap, int ncell, int cell_cap);
size_t mpp_chain_hbm_lds_bytes(int spec, int rowbase_n);
size_t mpp_deep_lds_bytes(int cap, int ncell, int cell_cap, int rowbase_n, int waves, int nmax, int ext);
hipError_t mpp_launch_chain(const ChainLaunch &a, int spec, int lanes, int occ);
hipError_t mpp_launch_chain_hbm(const ChainLaunch &a, int waves, unsigned char *ws, size_t ws_stride);
hipError_t mpp_launch_deep(const ChainLaunch &a, int waves, int occ, int nmax, int fixed_depth, int gain8, int flags,
                           unsigned long long *stats, int ext, const PreTab *pt);
hipError_t mpp_launch_hot(const ChainLaunch &a, const PreTab *pt);
hipError_t mpp_prepass_count(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile0, int n_chains,
                             const long long *until, unsigned long long seed, unsigned int chain0, int nblk, long long stride,
                             unsigned int *cnt, unsigned long long *total, unsigned int *qcnt, unsigned long long *qtot);
hipError_t mpp_prepass_fill(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile0, int n_chains,
                            const long long *until, unsigned long long seed, unsigned int chain0, int nblk, long long stride,
                            const unsigned int *off, uint32_t *word, double *rec, const unsigned int *qcnt, uint32_t *qoff,
                            QEnt *qent, long long *base);
void mpp_launch_papangelou_tiles(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_tiles, int max_n, int cap,
                                 double *dE, const int32_t *grid_start, const int32_t *grid_items, int sstride, int istride);
void mpp_launch_grid_build_all(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_tiles, int max_n, int ncell,
                               int cap, int32_t *start, int32_t *cursor, int32_t *items);
void mpp_launch_dedupe_tiles(hipStream_t st, const TileRef *tiles, int n_tiles, int max_n, int cap, const double *dE, long long dist2,
                             int32_t *work, int32_t *slot_of, int32_t *tx, int32_t *ty, double *ts, double *tr, double *ta,
                             int32_t *n_removed);
void mpp_launch_remap_table(hipStream_t st, const float *m, size_t n, double coef, double icpt, double *out);
void mpp_launch_set_until(hipStream_t st, const TileRef *tiles, int tile0, int n, long long n_steps, long long *until);
void mpp_launch_delta_vectors(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile, int n_cases,
                              const int32_t *rem_off, const int32_t *rem, const int32_t *add_off, const int32_t *add_xy,
                              const double *add_marks, int stride, double *before, double *after, unsigned char *mask,
                              const int32_t *grid_start, const int32_t *grid_items);
void mpp_launch_grid_build(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile, int n, int ncell, int32_t *start,
                           int32_t *cursor, int32_t *items);
int mpp_launch_affine_relu(hipStream_t st, void *x, int planes, int C, size_t hw, int elem_bytes, const float *scale,
                           const float *shift);
int mpp_launch_nhwc_glue(hipStream_t st, const void *x0, const void *x1, void *y, int H, int W, int C0, int C1, int pad, int pool,
                         int in_bytes, int out_bytes, const float *scale, const float *shift);
int mpp_launch_conv3x3_c32(hipStream_t st, const float *x0, const float *x1, int H, int W, const float *wp, const float *in_scale,
                           const float *in_shift, const float *out_scale, const float *out_shift, int relu, float *y);
int mpp_launch_conv3x3_stem(hipStream_t st, const float *x, int H, int W, const float *wp, const float *scale, const float *shift,
                            float *y);
void mpp_launch_quad_iou(hipStream_t st, int n, const double *a, int m, const double *b, double *out);
void mpp_launch_pack_detections(hipStream_t st, const TileRef *tiles, int n_tiles, const int32_t *tile_ids,
                                const int32_t *anchors, int capacity, double *out);
void mpp_launch_point_energies(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile, int n, double *e_pts,
                               double *vectors, const int32_t *grid_start, const int32_t *grid_items);
void mpp_launch_chain_energies(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_chains, int cap, double *e_pts,
                               double *energy, const int32_t *grid_start, const int32_t *grid_items, int sstride, int grid_min);
void mpp_launch_delta_batch(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile, int n_cases,
                            const int32_t *rem_off, const int32_t *rem, const int32_t *add_off, const int32_t *add_xy,
                            const double *add_marks, double *dE, const int32_t *grid_start, const int32_t *grid_items);
// the birth-energy map (mpp_birth_map.hip).  bc: the per-point cache, [n_chains][cap] each, filled by the pre-pass from the
// chains' grids (those of mpp_launch_grid_build_all; nullptr: every chain scans); dE [n_chains][H][W], marks the same x 3 or
// nullptr.  The summary: part [n_chains][MPP_BIRTH_PARTS] scratch, out [n_chains], all device.
void mpp_launch_birth_prepass(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_chains, int cap, BirthCache bc,
                              const int32_t *grid_start, const int32_t *grid_items, int sstride, int grid_min);
void mpp_launch_birth_map(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_chains, int cap, int H, int W,
                          BirthCache bc, double *dE, double *marks);
void mpp_launch_birth_summary(hipStream_t st, int n_chains, int H, int W, const double *dE, BirthPart *part,
                              mpp_birth_summary *out);
// the selection of local minima and the birth half of a round (mpp_birth_complete.hip).  mpp_launch_minsel: from the maps to
// n_cand, n_kept, keep and kblk; _emit: the kept pixels and values of chain t to xy / values + t * out_cap, out_cap >= every
// n_kept; _complete_append: an open chain's kept candidates go behind its configuration when they fit cap, their values to
// gain_val [n_chains][cap].  The count and the book are mpp_launch_descent_round's.
size_t mpp_minsel_bytes(int n_chains, int H, int W);
void mpp_minsel_plan(MinSel *s, void *ws);
void mpp_launch_minsel(hipStream_t st, const MinSel &s);
void mpp_launch_minsel_emit(hipStream_t st, const MinSel &s, int out_cap, int32_t *xy, double *values);
void mpp_launch_complete_append(hipStream_t st, const MinSel &s, const DevParams *P, const TileRef *tiles, int cap, double *gain_val);
// the exchange of parallel tempering at absolute step s, exchange number e (mpp_tempering.hip), all device: tiles the ctx's
// table (entry i: replica 0 of tile i, whose key the draw takes), sched [n_chains][3], rung [n_chains], energy [n_chains];
// accepted [n_maps][R - 1] counts per (tile, pair); log nullptr or log_cap records, this exchange's from log_base on
void mpp_launch_exchange(hipStream_t st, const TileRef *tiles, int n_maps, int R, double *sched, int32_t *rung, const double *energy,
                         long long s, long long e, unsigned long long seed, unsigned int chain0, long long *accepted,
                         mpp_exchange_record *log, long long log_base, long long log_cap);
// the recombination of restarts (mpp_recombine.hip), all device.  Recomb: the workspace of one call, placed by
// mpp_recombine_plan in mpp_recombine_bytes bytes.  mpp_launch_recombine: from the point energies e_pts [n_chains][cap] and
// chain energies e_sum [n_chains] (those of mpp_launch_chain_energies) to the written winner chains, rep and src; a tile of
// more than lds_points points over its replicas labels in the workspace.  _after: E_after of every report from the chain
// energies of the written state.
struct Recomb {
  int n, R, cap;                                   // tiles, replicas, point capacity
  int32_t *off;                                    // [n][R + 1] where a replica's points start in the tile's compact order
  int32_t *lab, *choice; uint32_t *xy; double *chosen;   // [n][R * cap] labels, packed positions, and per cluster root its replica and sum
  int32_t *spx, *spy; double *sps, *spr, *spa;     // [n][cap] the staged composite
  int32_t *src;                                    // [n][cap][2]
  mpp_recombine_report *rep;                       // [n]
};
size_t mpp_recombine_bytes(int n, int R, int cap);
void mpp_recombine_plan(Recomb *rc, int n, int R, int cap, void *ws);
void mpp_launch_recombine(hipStream_t st, const DevParams *P, const TileRef *tiles, const Recomb &rc, const double *e_pts,
                          const double *e_sum, int lds_points);
void mpp_launch_recombine_after(hipStream_t st, const Recomb &rc, const double *e_sum);
// the local descent (mpp_descent.hip), all device.  PtSel: one selection among points -- of the chains of `tiles` (their
// values and keep bytes `pitch` entries apart; a chain whose closed[] status is >= 0 has no candidates), or, tiles == nullptr,
// of one list of n points at x[i * stride], y[i * stride]; count: nullptr or two zeroed ints, candidates and kept.
struct PtSel {
  const TileRef *tiles; int n_chains, cap;
  const int32_t *x, *y; int stride, n;
  const double *val; uint8_t *keep; size_t pitch;
  double above, d2;
  const mpp_descent_report *closed;
  int32_t *count;
};
// The workspace of one mpp_descend / mpp_birth_complete, placed by mpp_descent_plan in mpp_descent_bytes bytes (hw: the pixels
// of a map, 0 without births).  _round (after the halves' launches) books the round; n_kept: MinSel::n_kept, nullptr without births.
struct Descent {
  int n_chains, cap;
  double *p, *rem_val, *gain_val;                  // [n_chains][cap]: Papangelou values; the removed p and the appended dE of a round by place
  double *dE;                                      // [n_chains][hw] the maps
  mpp_descent_report *rep;                         // [n_chains] the chain's one book; status >= 0: the chain is closed
  int32_t *src;                                    // [n_chains][cap]: where a slot's point started
  int32_t *n_rem;                                 // [n_chains] points the round's death half removed
  uint8_t *keep;                                   // [n_chains][cap] the selection's answer: 1 = remove
};
size_t mpp_descent_bytes(int n_chains, int cap, size_t hw);
void mpp_descent_plan(Descent *d, int n_chains, int cap, size_t hw, void *ws);
void mpp_launch_ptsel(hipStream_t st, const PtSel &s);
void mpp_launch_descent_init(hipStream_t st, const TileRef *tiles, const Descent &d);
void mpp_launch_descent_remove(hipStream_t st, const TileRef *tiles, const Descent &d);
void mpp_launch_descent_round(hipStream_t st, const TileRef *tiles, const Descent &d, int what, int max_rounds, const int32_t *n_kept);
void mpp_launch_descent_summary(hipStream_t st, const TileRef *tiles, const Descent &d, const mpp_birth_summary *sum_or_null);
// the relocation (mpp_relocate.hip), all device.  Move: the workspace of one mpp_move_gains / mpp_relocate, placed by
// mpp_move_plan in mpp_move_bytes bytes; the gains, the selection's answer, the round's list and the chains' closed flags are
// the Descent's (p, keep, rem_val / n_rem, rep[].status).  _move_gains: the pre-pass from the chains' grids (nullptr: every
// chain scans) and the gain kernel, into d.p and m.to; a chain whose d.rep status is >= 0 is skipped when `skip_closed`.
// _move_init after mpp_launch_descent_init; _move_apply after mpp_launch_ptsel rewrites the kept points and lists their gains;
// _move_round books the round; _move_finish after mpp_launch_descent_summary copies the summary into the books.
struct Move {
  int n_chains, cap;
  double *lin, *e, *best[MPP_MAX_PAIR], *second[MPP_MAX_PAIR];   // [n_chains][cap] the pre-pass's record of a point
  int32_t *gate, *slot[MPP_MAX_PAIR];              // ... its gate and, per pair term, the slot of the best value (-1: the seed)
  mpp_relocate_report *rep;                        // [n_chains] the chain's book
  int32_t *to;                                     // [n_chains][cap][2] the pixel of a point's best gain
  int32_t *moved;                                  // [n_chains][cap] how often a slot was rewritten
};
size_t mpp_move_bytes(int n_chains, int cap);
void mpp_move_plan(Move *m, int n_chains, int cap, void *ws);
void mpp_launch_move_gains(hipStream_t st, const DevParams *P, const TileRef *tiles, const Move &m, const Descent &d, int radius,
                           const int32_t *grid_start, const int32_t *grid_items, int sstride, int grid_min, int skip_closed);
void mpp_launch_move_init(hipStream_t st, const TileRef *tiles, const Move &m);
void mpp_launch_move_apply(hipStream_t st, const DevParams *P, const TileRef *tiles, const Move &m, const Descent &d);
void mpp_launch_move_round(hipStream_t st, const TileRef *tiles, const Move &m, const Descent &d, int max_rounds);
void mpp_launch_move_finish(hipStream_t st, const Move &m, const Descent &d);
void mpp_launch_cdf(hipStream_t st, int n_tiles, const float *det, int H, int W, double *rowpart, double *rowbase,
                    double *scratch_rowtot);
void mpp_launch_boxsum(hipStream_t st, int n_tiles, const double *rowpart, int H, int W, int md, double *boxsum);
void mpp_launch_rowwin(hipStream_t st, int n_tiles, const double *rowpart, int H, int W, int md, double *rowwin);
void mpp_launch_naive_init(hipStream_t st, const DevParams *P, const TileRef *tiles, int n_tiles, double threshold,
                           double nms_dist, unsigned long long *cand, int cand_cap);
// the U-Net epilogues: the window (wx0, wy0, wh x ww) of an H x W crop into dst, row pitch ld_dst pixels (mpp_maps.hip, mpp_conv.hip)
void mpp_launch_posnet_epilogue(hipStream_t st, const float *out, int H, int W, int ldh, int ldw, float w, float b, int wx0,
                                int wy0, int wh, int ww, float *dst, int ld_dst);
int mpp_launch_shapenet_epilogue(hipStream_t st, const float *logits, int ldh, int ldw, int wx0, int wy0, int wh, int ww,
                                 float *dst, int ld_dst);
int mpp_launch_posnet_epilogue_nhwc(hipStream_t st, const void *out, int elem_bytes, int H, int W, int ldw, float w, float b,
                                    int wx0, int wy0, int wh, int ww, float *dst, int ld_dst);
int mpp_launch_shapenet_epilogue_nhwc(hipStream_t st, const void *logits, int elem_bytes, int ldw, int wx0, int wy0, int wh,
                                      int ww, float *dst, int ld_dst);
int mpp_launch_shapenet_heads(hipStream_t st, const float *h, int ldw, const float *wh, const float *bh, int wx0, int wy0,
                              int wh_, int ww, float *m0, float *m1, float *m2, int ld_dst);
// the result pictures (mpp_figures.hip): every pointer device; owner [H][W] int32, used (and zeroed) only when n > 0
#define MPP_FIG_COORD_MAX (1 << 20)                // corner coordinates lie within +- this: the walk's arithmetic stays in int32
hipError_t mpp_launch_draw_outlines(hipStream_t st, int H, int W, const float *rgb, const float *scalar, double vmin, double vmax,
                                    const float *lut, int n, const int32_t *corners, const float *colors, int32_t *owner,
                                    uint8_t *out);
}
