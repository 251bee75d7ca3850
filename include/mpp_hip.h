/*
 * mpp_hip.h -- C ABI of libmppgpu.so, the MI355X (gfx950) implementation of the
 * MPP / RJMCMC sampling path of Ayana-Inria/MPP_CNN_RS_object_detection.
 *
 * The reference has no FFI: its boundary is a set of Python call signatures.
 * Each entry point below names the reference interface it stands behind
 * (paths relative to the reference repository root).  The Python binding that
 * mirrors those signatures is mpp_cnn_rs_object_detection_amd/{hip_api,point_set,sampler}.py;
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - every call returns 0 on success, <0 on error; mpp_last_error(ctx) has the text;
 *  - the caller owns every host buffer; the library owns device memory for the
 *    lifetime of the ctx; pointers passed with on_device=1 are borrowed, never freed;
 *  - a ctx is bound to one GPU and one HIP stream and is not thread-safe; distinct
 *    ctxs are independent; no global state, no callbacks, no Python objects;
 *  - a ctx holds n_tiles independent tiles of identical H x W ("tiles" are the
 *    reference's 256-px patches, models/mpp/mpp_model.py:231-248); one workgroup
 *    samples one tile.
 *  - "slot": points of a tile are kept in dense slots 0..n-1 (birth appends, death
 *    moves the last slot into the hole, move/transform rewrites in place).
 */
#ifndef MPP_HIP_H
#define MPP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what this header declares is exported */
#pragma GCC visibility push(default)

#define MPP_MAX_UNIT 8
#define MPP_MAX_PAIR 2
#define MPP_NCLASS 32
#define MPP_NKERNEL 10

/* unit energies: models/mpp/energies/data_energies.py, prior_energies.py */
enum {
  MPP_U_POSITION = 0,    /* p[0]=thr: -2*(det[x,y]-thr)                       data_energies.py:12-24   */
  MPP_U_SHAPE_REMAP = 1, /* p[0..2]=coef p[3..5]=icpt: mean_k(-2*sigmoid(coef_k*P_k+icpt_k)+1)
                            data_energies.py:27-45 + energy_setup_legacy.py:142-147                     */
  MPP_U_MARK_NEG = 2,    /* p[0]=k: -P_k[x,y,class_k]            energy_setup_no_calibration.py:68-80  */
  MPP_U_MARK_REMAP = 3,  /* p[0]=k p[1]=coef p[2]=icpt           (calib_marks=True)                     */
  MPP_U_AREA = 4,        /* p[0]=min p[1]=max: max(0,min-A,A-max)             prior_energies.py:53-67  */
  MPP_U_RATIO_PRIOR = 5, /* p[0]=target: |target-ratio|                       prior_energies.py:70-78  */
  MPP_U_CONST = 6,       /* p[0]=c (the unit energy of the reference's unit tests)                      */
  /* the classic image energies of the contrast setup (energy_setups/energy_setup_contrast.py:29-105): they read the
   * picture given with mpp_set_image, not a score map.  Chains with one of them run the extended kernel (spec_waves 1 or 8). */
  MPP_U_CONTRAST = 7,    /* p = {measure, dilation, gap, erode, thresh, fac, default_value}; measure: 0 lafarge, 1 craciun,
                            2 craciun2, 3 mean, 4 t-test, 5 debug: fac*measure(fill pixels, rim pixels) summed over the
                            channels - thresh                                  energies/classics.py:100-196 */
  MPP_U_GRADIENT = 8     /* p = {thresh, eps}: -|mean(grad . outline normal)| - thresh; the image holds np.gradient of
                            the picture, [H][W][C][2]                          energies/classics.py:199-235 */
};
/* pair energies: prior_energies.py */
enum {
  MPP_P_OVERLAP = 0,     /* area(P1^P2)/(min(A1,A2)+1e-6), reduce max         prior_energies.py:11-24  */
  MPP_P_ALIGN = 1,       /* 1-|cos(a1-a2)|-rewarding; p[0]=rewarding          prior_energies.py:27-50  */
  MPP_P_DIST_LE = 2,     /* [d<=max_dist]  (test/test_energy_graph.py:26-37)                            */
  MPP_P_DIST_LT = 3      /* [d< max_dist]  (test/test_interacting_points_set.py:30-42)                  */
};
enum { MPP_REDUCE_MAX = 0, MPP_REDUCE_MIN = 1 };
/* E(x) = sum_u F(lin0 + sum_k coef_k*g_k*v_k(u)); g_k=[v_gate<=gate_thr] if gated else 1.
 * F=identity: combination/hierarchical.py:13-48 and the plain sum of energy_graph.py:130-131;
 * F=2*sigmoid-1: combination/logistic.py:14-26. */
enum { MPP_C_LINEAR = 0, MPP_C_LOGISTIC = 1 };

typedef struct { int32_t kind, gated; double coef; double p[8]; } mpp_unit_term;
typedef struct { int32_t kind, gated, reduce, _pad; double coef, max_dist; double p[2]; } mpp_pair_term;

/* what EnergySetup.make_energies + an EnergyCombinationModel amount to
 * (energies/energy_setups/ and energies/combination/) */
typedef struct {
  int32_t n_unit, n_pair, combinator, gate_term;
  double gate_thr, lin0;
  mpp_unit_term unit[MPP_MAX_UNIT];
  mpp_pair_term pair[MPP_MAX_PAIR];
} mpp_model;

/* the three ValueMappings (models/shape_net/mappings.py:9-74): lower bin edges and ranges */
typedef struct {
  int32_t cyclic[3], _pad;
  double vmin[3], vmax[3];
  double edges[3][MPP_NCLASS];
} mpp_mappings;

/* kernel mixture, rjmcmc_sampler/kernels/make_kernels.py:50-177 (same order as its list) */
enum { MPP_K_UBIRTH = 0, MPP_K_UDEATH, MPP_K_DBIRTH, MPP_K_DDEATH, MPP_K_GTRANS, MPP_K_DTRANS,
       MPP_K_GTRANSF, MPP_K_DTRANSF,
       MPP_K_SPLIT, MPP_K_MERGE };   /* kernels/split_and_merge_kernels.py:40-178; p = 0 unless use_split_merge */
typedef struct {
  double p_kernel[MPP_NKERNEL];
  double sigma_trans;      /* 2   */
  double sigma_transform;  /* 0.1 */
  int32_t max_delta;       /* 8   */
  int32_t _pad;
  double split_radius;     /* 16  make_kernels.py:148 (SplitSampler.pos_radius = merge_radius) */
  double split_sigma;      /* 0.1 make_kernels.py:150 (x mark range) */
} mpp_kernels;

/* one fully specified proposal (tape replay); custom_types/perturbation.py:7-12 flattened */
typedef struct {
  int32_t kernel;
  int32_t target;          /* slot removed / moved, -1 if none.  Split: the split point, (aux0, aux1) = position
                            * delta, (as, ar, aa) = mark deltas.  Merge: target = p0, param_id = p1 (-1: none) */
  int32_t ax, ay;          /* proposed point */
  double as, ar, aa;
  double aux0, aux1;       /* raw normal deltas of the Gaussian kernels (Perturbation.data['delta']) */
  int32_t param_id, new_class;
  double u_accept;         /* the uniform of rjmcmc.py:113 */
} mpp_proposal;

/* per-step record; custom_types/rjmcmc.py:5-14 */
typedef struct {
  double dE, fwd, bwd, log_alpha, T;
  int32_t accepted, n_after;
} mpp_step_out;

typedef struct mpp_ctx mpp_ctx;

/* lifetime ------------------------------------------------------------------ */
int mpp_create(int device_id, mpp_ctx **out);
int mpp_destroy(mpp_ctx *ctx);
const char *mpp_last_error(mpp_ctx *ctx);
/* use an existing hipStream_t (e.g. torch's current stream); NULL = the ctx's own stream */
int mpp_set_stream(mpp_ctx *ctx, void *hip_stream);
int mpp_synchronize(mpp_ctx *ctx);
/* "spec_waves": proposals evaluated speculatively per round, one wave each (1 = strictly one at a
 * time); "spec_lanes" (0 = off): lane mode, 4 waves of which `v` lanes each evaluate one step on
 * their own, 4*v steps per round (overrides spec_waves); "deep" (default 128; 0 = off; a power of two in 8..256): deep
 * rounds -- every LANE of the chain's spec_waves waves evaluates one step, up to `v` (at most 64 * spec_waves) steps per
 * round, the steps sorted by kernel type across the workgroup, neighbour energies evaluated by the whole wave for all its
 * steps at once (csrc/mpp_deep.hip); used for chains drawn from Philox under the shipped energy setups (overlap / max +
 * alignment / min pair terms, no split / merge, no classic image energy), others run one wave per step as before;
 * "handover" (default 1): a chain of 8 waves starts with one wave per step and is handed to the deep rounds once about 6 of
 * 8 steps commit per round (a hot chain changes its state every few steps: short rounds suit it better); same chain;
 * "handover_at" (default 1280): that number of steps committed per round, x 256;
 * "handover_tiles" (default 64): only launches of at most this many chains start that way (the launch that hands over
 * ends when its last chain has cooled down);
 * "deep_fixed" (tests): a fixed number of steps per round instead of the adaptive depth; "deep_gain" (8..64, default 12):
 * the adaptive depth in eighths of the smoothed number of steps the last rounds committed; read-only "deep_stat0".."deep_stat3":
 * rounds, steps evaluated, rounds with a second pass, steps committed by the last mpp_run.  The chain is identical for every setting. "point_capacity": slots per tile (before mpp_set_maps, at most 65535: 16-bit slot indices), "cell_capacity" (points per
 * 32-px cell, at most 2048), "auto_grow" (default 1): a chain that would exceed either capacity stops BEFORE that step and
 * mpp_run / mpp_replay double the capacity and continue it -- the reference's point set has no capacity
 * (point_set/point_set.py:45-188); with 0 the call fails with -11 / -12 and the chain can be continued by hand from the
 * written-back state ("grow_events", read-only, counts the re-launches); "chain_state" (default 0, auto): a chain lives in
 * its workgroup's LDS (160 KB); one that outgrows it -- a capacity the LDS cannot hold, or a context whose capacities exceed
 * the LDS from the start -- continues with its state in device memory (the same chain, slower steps) while the other chains
 * of the call and of later calls stay in LDS; 1: LDS only (such a chain fails the call with -12 / -11, a context too large
 * for the LDS with -7); 2: every chain in device memory (tests, diagnosis); read-only "hbm_chains": chains that ran at
 * least one launch in device memory in the last mpp_run / mpp_replay, "hbm_bytes": the device workspace held for them;
 * -11 / -12 otherwise only remain at the limits of 2048 per cell and 65535 slots; "prepass" (default 1; 0 off): a deep
 * launch first draws the births of all its steps with a wide kernel and its chains load them (the same chain); a launch
 * whose table would exceed "prepass_mb" (default 256, 1..16384) runs without one; read-only "prepass_used": a deep launch
 * of the last mpp_run / mpp_replay used one; "replicas" (before mpp_set_maps): v independent chains per tile, chain t on the maps of
 * tile t % n_tiles; "remap_table" (-1 auto, default; 0 never; 1 always): chains of a model with the
 * MPP_U_SHAPE_REMAP term read the remapped mark probabilities from [H][W][32] float64 tables built once per mpp_set_maps (as
 * the reference does, energy_setup_legacy.py:142-147) instead of evaluating three sigmoids per proposal -- the same values bit
 * for bit; auto: while the tables fit 2 GB (a few tiles sampled long; for hundreds of tiles building them costs more than they save); reading it back tells whether they are in use; "force_accept": apply every proposal without the Metropolis test (the kernel random
 * walks of models/mpp/perturbation_sampler.py:152-169); "scratch_grid_min_points" (default 256; 0 = never): configurations of
 * at least that many points get a candidate grid (PointsSet.get_potential_neighbors, point_set.py:111-145) for
 * mpp_total_energy / mpp_delta_batch / mpp_delta_vectors / mpp_papangelou instead of a scan of all points.  Read-only: "n_chains", "lds_bytes", and the spatial-hash
 * geometry "grid_nx", "grid_ny", "grid_res" (point_set/point_set.py:58-61) */
int mpp_set_option(mpp_ctx *ctx, const char *name, int64_t value);
int64_t mpp_get_option(mpp_ctx *ctx, const char *name);

/* score maps: ImageWMaps.detection_map / param_dist_maps (custom_types/image_w_maps.py:11-22).
 * det: [n_tiles][H][W] float32; m0..m2: [n_tiles][H][W][32] float32 (size, ratio, angle). */
int mpp_set_maps(mpp_ctx *ctx, int n_tiles, int H, int W, const float *det, const float *m0,
                 const float *m1, const float *m2, int on_device);
/* the picture the classic image energies read (ImageWMaps.image, custom_types/image_w_maps.py:11-22, as prepared by
 * ContrastEnergy.__post_init__ / GradientEnergy.__post_init__, classics.py:113-149, :207-215): img [n_tiles][H][W][C]
 * float32, after mpp_set_maps (same n_tiles, H, W); C = 1 or 3 for MPP_U_CONTRAST, 2 or 6 (np.gradient, [..][C/2][2]) for
 * MPP_U_GRADIENT.  on_device: borrowed.  Dropped by the next mpp_set_maps. */
int mpp_set_image(mpp_ctx *ctx, int n_tiles, int C, const float *img, int on_device);
int mpp_set_model(mpp_ctx *ctx, const mpp_model *model, const mpp_mappings *mappings);
/* make_kernels(image_data, intensity, rng): intensity[n_tiles] = max(1,len(init)) (sample_rjmcmc.py:68) */
int mpp_set_kernels(mpp_ctx *ctx, const mpp_kernels *kernels, const double *intensity);

/* EPointsSet (point_set/energy_point_set.py:18-166) ---------------------------- */
int mpp_set_points(mpp_ctx *ctx, int tile, int n, const int32_t *xy, const double *marks);
int mpp_get_points(mpp_ctx *ctx, int tile, int cap, int32_t *n, int32_t *xy, double *marks);
int mpp_count(mpp_ctx *ctx, int tile, int32_t *n);
/* all tiles at once (the per-tile results `Pool.map` hands back, mpp_model.py:250-262): n[n_tiles]; if xy and marks are
 * not NULL, xy [n_tiles][cap][2] and marks [n_tiles][cap][3] receive the first min(n[t], cap) points of every tile */
int mpp_get_points_all(mpp_ctx *ctx, int cap, int32_t *n, int32_t *xy, double *marks);
/* The configurations of tiles 0..n-1 of the ctx packed into ONE fixed-capacity record buffer ON THE DEVICE: the send
 * buffer of the all-gather (RCCL over xGMI) that stands in for the result list `Pool.map` returns in
 * mpp_model.py:250-262.  out_dev [capacity+1][7] float64 (device pointer of this ctx's GPU): row 0 = (count, 0...),
 * row 1+k = (tile_ids[t], x + anchors[t][0], y + anchors[t][1], size, ratio, angle, 0) -- image coordinates as
 * merge_patches forms them (data_loaders.py:133-138), tiles in order, points in slot order; the rest is zeroed.
 * tile_ids [n], anchors [n][2]: host arrays.  count (may be NULL) receives the number of records; -4 if > capacity. */
int mpp_pack_detections(mpp_ctx *ctx, int n, const int32_t *tile_ids, const int32_t *anchors, int capacity,
                        double *out_dev, int32_t *count);
/* total_energy(): combined energy and, optionally, [n][n_unit+n_pair] per-point vectors */
int mpp_total_energy(mpp_ctx *ctx, int tile, double *energy, double *vectors_or_null);
/* total_energy() of every chain of the ctx at once (n_chains = tiles x "replicas"), from the state the last mpp_run /
 * mpp_set_points left (the state mpp_get_points_all reads): energy [n_chains], energy[t] bit for bit what
 * mpp_total_energy(ctx, t, ..) returns (the same kernel, the points summed in slot order on the device), 0.0 for an empty
 * chain.  A fixed number of launches, one copy of n_chains doubles and one synchronise, however many chains; honours
 * "scratch_grid_min_points".  What the choice among restarts reads (sampler.select_replicas). */
int mpp_total_energy_all(mpp_ctx *ctx, double *energy);
/* The per-point energies behind mpp_total_energy_all, from the same launches: e HOST [n_chains][point_capacity],
 * e[c][s] = e(point in slot s of chain c | the chain's configuration) for s < n_c, 0.0 behind n_c.  Row c added up in slot
 * order from 0.0 is energy[c] of mpp_total_energy_all, bit for bit.  The same refusals. */
int mpp_point_energies_all(mpp_ctx *ctx, double *e);
/* energy_delta(Perturbation) for a batch of perturbations with list removals/additions:
 * case i removes slots rem[rem_off[i]..rem_off[i+1]) and adds rectangles add_off[i]..add_off[i+1] */
int mpp_delta_batch(mpp_ctx *ctx, int tile, int n_cases, const int32_t *rem_off, const int32_t *rem,
                    const int32_t *add_off, const int32_t *add_xy, const double *add_marks, double *dE);
/* The same perturbations, but the per-point energy VECTORS (n_unit unit terms, then n_pair reductions) before and
 * after each one instead of the combined dE: what EnergyComputeTorch.compute feeds to the torch weight model in
 * train_energy_combination/train_ordering_criterion.py:27-40,101-118 (via energy_graph.py:139-225).
 * Row i*stride + j of before/after ([n_cases*stride][n_unit+n_pair]) and mask ([n_cases*stride]): j < n is
 * existing slot j, j >= n the (j-n)-th rectangle added by case i; stride >= n + additions of every case.
 * mask: 0 untouched, 1 neighbour of a change (both rows valid), 2 removed (before only), 3 added (after only). */
int mpp_delta_vectors(mpp_ctx *ctx, int tile, int n_cases, const int32_t *rem_off, const int32_t *rem,
                      const int32_t *add_off, const int32_t *add_xy, const double *add_marks, int stride,
                      double *before, double *after, unsigned char *mask);
/* papangelou(u, remove_u_from_point_set=True, return_energy_delta=True) of every point */
int mpp_papangelou(mpp_ctx *ctx, int tile, double *dE);
/* merge_patches(..., method='distance', distance) of models/mpp/data_loaders.py:122-161 and the two scorings around it
 * (mpp_model.py:296-304), for EVERY tile of the ctx at once: a tile holds the aggregated detections of one image (mpp_set_points)
 * on that image's score maps.  On the device: the Papangelou intensity of every point in its tile's configuration; the walk
 * of data_loaders.py:140-159 -- in index order every not-yet-removed point keeps, among the not-yet-removed points within
 * `distance` of it, only the one with the best intensity (scores equal to 1e-9 tie, the first wins) --; the removals in the
 * order EPointsSet.remove leaves (the last point takes the hole); the Papangelou values of the survivors.  The tiles'
 * configurations ARE the survivors afterwards.  n_out [n_tiles], xy [n_tiles][cap][2], marks [n_tiles][cap][3], dE
 * [n_tiles][cap] = E(with u) - E(without u) (score = exp(-dE)), n_removed [n_tiles] (may be NULL).  -4: a tile holds more
 * points than the device walk takes (8192): merge that image on the host. */
int mpp_merge_score(mpp_ctx *ctx, double distance, int cap, int32_t *n_out, int32_t *xy, double *marks, double *dE,
                    int32_t *n_removed);
/* The birth-energy map: for every pixel c = (x, y) of every chain t of the ctx, the energy change of adding the rectangle
 * ShapeNet proposes there, dE(c) = E(X + u_c) - E(X) -- the conditional (Papangelou) intensity surface exp(-dE) of the
 * point process, evaluated where there is NO detection (the reference's utils/figures/ show_papangelou).  X is the state
 * mpp_get_points_all reads (after mpp_set_points or mpp_run), on the maps of tile t % n_tiles.
 *   candidate  u_c = (x, y, edges[0][c0], edges[1][c1], edges[2][c2]) with ck the argmax class of mark map k at c by the rule of
 *              mpp_mark_classes (first maximum, a NaN wins) and edges the lower bin edges of mpp_mappings
 *              (ValueMapping.class_to_value, cnn_detection.mark_values);
 *   value      dE(c) = e(u_c | X + u_c) + sum over the slots v with d(v, c) <= max_inter of [ e(v | X + u_c) - e(v | X) ],
 *              every e(. | .) the point energy of mpp_total_energy / mpp_delta_batch for that point in that configuration;
 *   order      the neighbour differences are added in ASCENDING SLOT ORDER to a float64 that starts at 0.0, then e(u_c | .)
 *              is added: a pixel's value does not depend on launch shape, number of tiles or replicas, bit for bit;
 *   a point already on c is a neighbour like any other (d = 0).
 * The pair reductions are max / min, so red_v(X + u_c) = reduce(red_v(X), pair(v, u_c)) is the from-scratch reduction bit for
 * bit: a pre-pass caches every point's unit part, reductions and energy in X (workspace of the ctx, grown on demand; it
 * honours "scratch_grid_min_points"), the map kernel stages the cached points near a block of pixels in LDS,
 * MPP_BIRTH_CHUNK at a time, and walks them in slot order.
 * dE [n_chains][H][W] float64 and marks_or_null [n_chains][H][W][3] float64 (the candidates' size, ratio, angle): DEVICE
 * pointers, borrowed; summary_or_null [n_chains]: HOST.  Runs on the ctx's stream; returns when summary (if given) is filled,
 * otherwise asynchronous.  Summary of a chain: min_dE the smallest non-NaN value (finite or infinite), (x, y) its pixel, ties
 * to the smallest row-major index x * W + y; n_negative the pixels with dE < 0; n_nan the pixels whose value is NaN; all
 * values NaN: min_dE = +inf, (x, y) = (-1, -1).
 * -1 with a message: no maps or no model; a model with a classic image energy (MPP_U_CONTRAST, MPP_U_GRADIENT: a candidate per
 * pixel would need a rasterised footprint per pixel); more than 65535 chains.  The kernel mixture is not read.
 * Read-only option "birth_map_grid": the last call's pre-pass built candidate grids (its chains of at least
 * "scratch_grid_min_points" points took their neighbours from them, the others scanned). */
#define MPP_BIRTH_CHUNK 256        /* points staged per pass of a block */
typedef struct { double min_dE; int32_t x, y; int64_t n_negative, n_nan; } mpp_birth_summary;
int mpp_birth_energy_map(mpp_ctx *ctx, double *dE, double *marks_or_null, mpp_birth_summary *summary_or_null);
/* The local minima of a float64 map below a level (csrc/mpp_birth_complete.hip): dE_dev [H][ld] float64, xy [cap][2] int32
 * (row, col) and values [cap] float64 are DEVICE pointers; n_candidates / n_kept are host pointers (either may be NULL); the
 * ctx's stream, synchronous.
 *  - candidates: the pixels with dE < below.  A NaN never is one, -inf is;
 *  - key: key(c) = (dE(c), x * W + y), compared lexicographically: equal values (-inf included) tie toward the smaller
 *    row-major index;
 *  - kept: a candidate c is kept iff no OTHER candidate c' with (double)(dx*dx + dy*dy) <= distance * distance has
 *    key(c') < key(c).  The rule does not depend on an order of visits (it is not the rank-order NMS of mpp_detect_centers):
 *    a candidate that loses to a neighbour which itself loses is dropped too -- callers that repeat the selection give it
 *    its turn in a later round.  A non-candidate never beats a candidate: this is the minimum filter over the disc;
 *  - output: the kept pixels and their values in ASCENDING ROW-MAJOR ORDER.  If more than cap are kept: -13, *n_kept = the
 *    number needed, nothing written to xy / values.
 * The candidates are compacted by ballot into a list in a workspace of the ctx (12 B per pixel at most, grown on demand) and
 * resolved among the list only.  -1: distance < 0, a non-finite distance or below, ld < W, H*W >= 2^31, H or W < 1. */
int mpp_select_minima(mpp_ctx *ctx, int H, int W, int ld, const double *dE_dev, double below, double distance, int cap,
                      int32_t *xy, double *values, int64_t *n_candidates, int64_t *n_kept);
/* Greedy completion: births from the birth-energy map until none lowers the energy by more than min_gain.  Every chain of the
 * ctx on its own, from the state mpp_get_points_all reads.  A round:
 *   the map of mpp_birth_energy_map of the current state (into the workspace of mpp_descend, whose births-only round loop
 *   this is: 8 B per pixel per chain);
 *   mpp_select_minima on it with below = -min_gain and distance = 2 * max_inter, max_inter the model's largest pair range --
 *   two kept candidates then neither interact nor share a neighbour, so in real arithmetic the round lowers the energy by
 *   exactly the sum of its dE;
 *   the kept candidates u_c (the map's candidates: position c, marks edges[k][argmax class]) are appended to the chain's
 *   configuration in slots n .. n+k-1, ascending row-major order.  The chain is then in the state mpp_set_points(old + new)
 *   leaves.  Nothing crosses to the host but one record per chain and round.
 * status 0: a round kept nothing (converged); 1: max_rounds rounds have appended points (1 <= max_rounds <= 1024); 2: the
 * points of a round do not fit point_capacity -- nothing of that round is appended to that chain, the other chains go on.
 * rounds: the rounds that appended points; n_added their points; n_after the chain's count; gain the sum of the appended dE,
 * added one after another to a float64 that starts at 0.0, round by round and in slot order within a round; min_dE, x, y,
 * n_negative, n_nan: the mpp_birth_summary of the map of the RETURNED state (after status 1 one more map is computed).
 * report [n_chains]: HOST.  -1 with a message: max_rounds outside 1..1024, min_gain negative or not finite, and the refusals of
 * mpp_birth_energy_map (no maps or no model; a classic image energy; more than 65535 chains). */
typedef struct { int32_t status, rounds, n_added, n_after; double gain, min_dE; int32_t x, y; int64_t n_negative, n_nan; } mpp_complete_report;
int mpp_birth_complete(mpp_ctx *ctx, int max_rounds, double min_gain, mpp_complete_report *report);
/* Recombination of restarts (csrc/mpp_recombine.hip): per tile, the best replica PER INTERACTION
 * CLUSTER instead of the best replica as a whole.  n = n_chains / "replicas" tiles, R = "replicas" >= 2, chain r * n + i is
 * replica r of tile i; the state is the one mpp_get_points_all reads.  All on the ctx's stream; only the reports and src
 * cross to the host.  The rules, such that a restatement on the host matches every output exactly:
 *   1. energies  the launches of mpp_total_energy_all: per-point e and per-chain sums, the same bits ("scratch_grid_min_points"
 *                is honoured).
 *   2. winner    w_i, the rule of sampler.select_replicas: start at replica 0; replica r replaces the best when its chain
 *                energy is strictly lower, or when the best is not finite and r's is.
 *   3. link      two points of the tile -- of any two replicas, or of the same one -- are linked iff
 *                sqrt((double)dx*dx + (double)dy*dy) <= max_inter in float64, the "interacts" test of the energy kernels
 *                (points_interact, csrc/mpp_scratch.hpp).  Coincident points are linked.
 *   4. cluster   a connected component of the links; its id is the smallest global index g = r * point_capacity + slot among
 *                its members.  (Min-label propagation with pointer jumping, one workgroup per tile, until a sweep changes
 *                nothing; the labels live in LDS while the tile's points over all replicas number at most
 *                "recombine_lds_points", default and upper limit MPP_RECOMBINE_LDS_POINTS, else in a workspace of the ctx.)
 *   5. sums      S[r][C] = the sum of e over replica r's members of C in ascending slot order, float64 from 0.0; a replica
 *                without a member in C has S = 0.0 and competes like any other.
 *   6. choice    best = w_i; for r = 0 .. R-1, r != w_i: r is taken when S[r][C] < S[best][C], or when S[best][C] is not
 *                finite and S[r][C] is.  Ties stay with the winner.
 *   7. composite replicas in the order w_i, then 0 .. R-1 without w_i, slots ascending within a replica; a point is kept iff
 *                its cluster chose its replica.  The m_i kept points go to slots 0 .. m_i-1 of chain w_i * n + i (positions,
 *                marks, count, error code 0): the state mpp_set_points(composite) leaves.  Staged through a workspace.  Every
 *                other chain, and every schedule, key, step counter and intensity, is untouched.
 *   8. status    0: no cluster chose another replica -- nothing is written, the winner chain keeps its bytes; 1: recombined;
 *                2: m_i > point_capacity -- nothing is written for that tile, the other tiles go on.
 *   9. report    status, winner; n_clusters, n_taken (clusters that chose r != w_i); n_before / n_after: the count of chain
 *                w_i * n + i before / after the call; E_winner: that chain's energy (rule 1); E_sum: the chosen S added in
 *                ascending cluster id, float64 from 0.0 (whatever the status); E_after: the launches of rule 1 once more on
 *                the written state -- mpp_total_energy(ctx, w_i * n + i, ..) bit for bit, E_winner for status 0 and 2.
 *  10. src       src_or_null HOST [n][point_capacity][2] int32: src[i][k] = (replica, slot) composite slot k came from, for
 *                k < n_after; for status 0 and 2 that is (w_i, k); (-1, -1) behind n_after.
 * Every point of X* keeps the neighbours it had in its replica and gains none (both lie in its cluster), and the pair
 * reductions are max / min, so e(v | X*) = e(v | X_r(C)) bit for bit and, in real arithmetic, E_after = E_sum <= E_winner.
 * report HOST [n].  -1 with a message: no maps or no model; "replicas" < 2; more than 65535 chains.  A model with a classic
 * image energy is allowed (its unit terms are per point); a reduction that is not MPP_REDUCE_MAX / MPP_REDUCE_MIN is refused. */
#define MPP_RECOMBINE_LDS_POINTS 2048      /* points of a tile, over all replicas, whose labels fit the LDS */
typedef struct { int32_t status, winner, n_clusters, n_taken, n_before, n_after; double E_winner, E_sum, E_after; } mpp_recombine_report;
int mpp_recombine(mpp_ctx *ctx, mpp_recombine_report *report, int32_t *src_or_null);
/* Local descent (csrc/mpp_descent.hip): greedy deaths and births to a joint fixed point.
 *
 * mpp_papangelou_all: dE HOST [n_chains][point_capacity]; dE[c][s] = mpp_papangelou(ctx, c)[s] bit for bit for s < n_c and 0.0
 * behind n_c.  The launches of mpp_merge_score's scoring (the candidate grids when point_capacity reaches
 * "scratch_grid_min_points" -- with or without them the bits are the same --, then the Papangelou kernel over every chain) and
 * one copy back.  Refuses what mpp_total_energy_all refuses.
 *
 * mpp_select_points: the descent's selection on a caller's list of n points; xy_dev [n][2] int32, values_dev [n] float64 and
 * keep_dev [n] uint8 are DEVICE pointers, n_candidates / n_kept HOST (either may be NULL); the ctx's stream, synchronous.
 *  - candidates: the points with values[i] > above.  A NaN never is one, +inf is;
 *  - key: key(i) = (-values[i], i): the larger value wins, equal values tie toward the smaller slot;
 *  - kept: a candidate is kept iff no OTHER candidate j with (double)(dx*dx + dy*dy) <= distance * distance (dx, dy 64-bit
 *    integers) has a smaller key.  Two points on one pixel are rivals.  Order-free as mpp_select_minima: a candidate that loses
 *    to a loser is dropped for this round;
 *  - keep[i] = 1 or 0 for every i < n.
 * -1: distance < 0, a non-finite distance or above, n < 0.
 *
 * mpp_descend: every chain of the ctx on its own, from the state mpp_get_points_all reads.  what: MPP_DESCEND_DEATHS,
 * MPP_DESCEND_BIRTHS or both.  A round:
 *   death half (bit 1)  p(v) = E(X) - E(X - v) of every point of the current state, the values of mpp_papangelou; the selection
 *                       above with above = min_gain and distance = 2 * max_inter; the kept points are REMOVED by stable
 *                       compaction (the survivors keep their relative slot order).  The chain is then in the state
 *                       mpp_set_points(survivors in slot order) leaves.  Two points removed in one round neither interact nor
 *                       share a neighbour, so in real arithmetic the half lowers the energy by exactly the sum of its p;
 *   birth half (bit 2)  one round of mpp_birth_complete on the state the death half left: the map, mpp_select_minima with
 *                       below = -min_gain and distance = 2 * max_inter, the append in ascending row-major order.
 * status 0: a whole round changed nothing -- a joint fixed point for min_gain; 1: max_rounds (1..1024) rounds have changed the
 * chain; 2: a birth half does not fit point_capacity -- nothing of that half is appended and the chain closes, what its death
 * half removed stays removed and counted (the round counts when it removed something); the other chains go on.  A closed
 * chain is not touched again.
 * report [n_chains] HOST: rounds = the rounds that changed the chain; n_added, n_removed, n_after; gain_births = the sum of the
 * appended dE, gain_deaths = the sum of the removed p, each a float64 from 0.0 to which the values are added one after another,
 * round by round and in slot order within a round.  Of the RETURNED state: max_p the largest non-NaN p and slot_max the first
 * slot that has it ((-inf, -1) for an empty chain or when every p is NaN), n_positive the count of p > 0, and -- when bit 2 is
 * set -- the mpp_birth_summary fields min_dE, x, y, n_negative, n_nan (without bit 2 no map is computed: 0.0, -1, -1, 0, 0).
 * After status 1 or 2 one more Papangelou pass, after status 1 one more map is computed for these fields.
 * src_or_null HOST [n_chains][point_capacity] int32: for every final slot the slot the point had when the call began, -1 for a
 * born point and behind n_after.
 * With what = MPP_DESCEND_BIRTHS the chain state and every shared report field equal those of mpp_birth_complete bit for bit.
 * Per round a fixed number of launches and one copy of n_chains reports; no point list and no map crosses to the host.
 * -1 with a message: what outside 1..3; max_rounds outside 1..1024; min_gain negative or not finite; a pair reduction that is
 * neither max nor min; more than 65535 chains; no maps or no model; with bit 2 a classic image energy (deaths alone are
 * allowed: the unit terms are per point).
 * The map's dE(c) and the from-scratch p of the same point are one real number in two summation orders: with min_gain = 0 a
 * point within rounding of 0 could be born and removed in turn; max_rounds ends that with status 1, a min_gain above the
 * rounding bound excludes it. */
#define MPP_DESCEND_DEATHS 1
#define MPP_DESCEND_BIRTHS 2
typedef struct {
  int32_t status, rounds, n_added, n_removed, n_after, slot_max;
  double gain_births, gain_deaths, max_p, min_dE;
  int32_t x, y;
  int64_t n_positive, n_negative, n_nan;
} mpp_descent_report;
int mpp_papangelou_all(mpp_ctx *ctx, double *dE);
int mpp_select_points(mpp_ctx *ctx, int n, const int32_t *xy_dev, const double *values_dev, double above, double distance,
                      uint8_t *keep_dev, int64_t *n_candidates, int64_t *n_kept);
int mpp_descend(mpp_ctx *ctx, int what, int max_rounds, double min_gain, mpp_descent_report *report, int32_t *src_or_null);
/* Relocation (csrc/mpp_relocate.hip): move a point to a better map candidate nearby, in one step.
 *
 * mpp_move_gains: for every point v (slot i) of every chain and every pixel c of the (2 radius + 1)^2 window around v, clipped
 * to the tile, with u_c the candidate of mpp_birth_energy_map at c (position c, marks edges[k][argmax class]):
 *   value   g(v, c) = E(X) - E(X - v + u_c), X' = X - v + u_c;
 *   order   S = e(u_c | X') - e(v | X), one difference; then e(w | X') - e(w | X) of the slots w != i within max_inter of v or
 *           of c is added to S one after another in ASCENDING SLOT ORDER; g = -S.  Every e(. | .) is the point energy of
 *           mpp_total_energy.  A pixel's g does not depend on the other chains, on n_chains, on "scratch_grid_min_points" or on
 *           the radius (beyond which pixels are in the window), bit for bit;
 *   output  gain[i] = the largest non-NaN g over the window, to[i] = (x, y) of its pixel, ties to the smaller row, then the
 *           smaller column; gain = NaN and to = (-1, -1) when every g is NaN.  c = v's own pixel is a candidate: it replaces
 *           the marks only.  Behind a chain's count: 0.0 and (-1, -1).
 * The pair reductions are max / min from the seed 0.0, exact selections: a pre-pass caches per point and pair term the best
 * value, the second-best and the slot of the best, so red_w(X - v) is the second-best when v is the slot of w's best and the
 * best otherwise (equal values: second = best; the seed is a contributor no removal takes away), and red_w(X') =
 * reduce(red_w(X - v), pair(w, u_c)).  One workgroup per point, one lane per window pixel; the points within reach are staged
 * in LDS in slot order, MPP_MOVE_CHUNK at a time, and walked twice: first for u_c's own reductions, then for the sum.
 * gain HOST [n_chains][point_capacity] float64, to HOST [n_chains][point_capacity][2] int32.  -1 with a message: radius
 * outside 1..MPP_MOVE_RADIUS_MAX; no maps or no model; a classic image energy (the candidate's unit terms come from the
 * maps); a pair reduction that is neither max nor min; more than 65535 chains.  Read-only option "move_gains_grid": the last
 * call's pre-pass built candidate grids.
 *
 * mpp_relocate: every chain of the ctx on its own, from the state mpp_get_points_all reads.  A round of an open chain:
 *   the gains above; the selection of mpp_select_points on them with above = min_gain and
 *   distance = 2 * (max_inter + radius * sqrt(2.0)) in float64; every kept point is REWRITTEN IN PLACE: position to[i], marks
 *   the candidate's there; slot, count and slot order stay, the error code is cleared when something moved -- the state
 *   mpp_set_points of the edited list leaves.
 * A move changes only points within max_inter of v or of c, and |v - c| <= radius * sqrt(2): two kept points, further apart
 * than the distance, neither interact before or after nor share an affected neighbour, so in real arithmetic a round lowers
 * the energy by exactly the sum of its gains.
 * status 0: a round moved nothing; 1: max_rounds (1..1024) rounds have moved something (the count never changes: there is no
 * status 2).  A closed chain is not touched again.  report [n_chains] HOST: rounds = the rounds that moved something; n_moved
 * the moves; n_after the chain's count; gain = the kept gains added one after another to a float64 from 0.0, round by round and
 * in slot order within a round.  Of the RETURNED state: max_gain the largest non-NaN gain and slot_max the first slot that has
 * it ((-inf, -1) for an empty chain or when every gain is NaN), n_positive the count of gains > 0; after status 1 one more gain
 * pass is computed for them.  moved_or_null HOST [n_chains][point_capacity] int32: how often a slot was rewritten, 0 behind
 * the count.  Per round a fixed number of launches and one copy of n_chains reports; no point list crosses to the host.
 * -1 with a message: the refusals of the gains; max_rounds outside 1..1024; min_gain negative or not finite; report NULL.
 * With min_gain = 0 a point within rounding of 0 could move back and forth between two pixels; max_rounds ends that with
 * status 1, a min_gain above the rounding bound excludes it. */
#define MPP_MOVE_CHUNK 256         /* points staged per pass of a workgroup */
#define MPP_MOVE_RADIUS_MAX 7      /* 15 x 15 = 225 window pixels in 256 lanes */
typedef struct { int32_t status, rounds, n_moved, n_after, slot_max, n_positive; double gain, max_gain; } mpp_relocate_report;
int mpp_move_gains(mpp_ctx *ctx, int radius, double *gain, int32_t *to);
int mpp_relocate(mpp_ctx *ctx, int radius, int max_rounds, double min_gain, mpp_relocate_report *report, int32_t *moved_or_null);
/* naive_detection (sample_rjmcmc.py:23-35): threshold + greedy distance-NMS, sets every tile's points.  Candidates are
 * det >= (float)threshold (float32, as NumPy compares); rank and NMS rule as mpp_detect_centers below.  A tile that keeps more
 * than point_capacity points: -12 ("naive init, tile t"), its first point_capacity picks stay stored; every call replaces
 * the tiles' configurations and error codes, so a later call that fits succeeds. */
int mpp_naive_init(mpp_ctx *ctx, double threshold, double nms_distance);

/* RJMCMC (rjmcmc_sampler/rjmcmc.py:52-187, sample_rjmcmc.py:38-102) ------------- */
int mpp_set_schedule(mpp_ctx *ctx, double T0, double alpha, double T_target);
/* replay n given proposals on one tile; out may be NULL */
int mpp_replay(mpp_ctx *ctx, int tile, int n, const mpp_proposal *tape, mpp_step_out *out);
/* n_steps of the chain on every tile at once; proposals from Philox4x32-10(key=seed,
 * ctr=(step, block, chain = chain0+tile)).  trace_tile>=0 records that tile's steps. */
int mpp_run(mpp_ctx *ctx, int64_t n_steps, uint64_t seed, uint32_t chain0, int trace_tile,
            mpp_step_out *out_or_null, mpp_proposal *props_or_null);
/* Per-chain Philox keys: chain t of the ctx draws its proposals from Philox4x32-10(key = seeds[t], ctr = (step, block,
 * chains[t])) instead of (the launch's seed, chain0 + t).  This is what lets the tiles of SEVERAL images share one launch --
 * the reference samples image after image (mpp_model.py:220-262), one kernel launch per image would leave most of the GPU
 * idle -- while every tile runs exactly the chain it would run in a launch of its own image.  n = number of chains of the
 * ctx; seeds == NULL or chains == NULL: back to mpp_run's arguments.  Reset by mpp_set_maps. */
int mpp_set_chain_keys(mpp_ctx *ctx, int n, const uint64_t *seeds, const uint32_t *chains);
int mpp_step_index(mpp_ctx *ctx, int tile, int64_t *step);
/* time of the last mpp_run / mpp_replay kernel in ms (HIP events on the ctx's stream); after mpp_run_tempered the sum over
 * its segments */
int mpp_last_kernel_ms(mpp_ctx *ctx, double *ms);

/* Parallel tempering (replica exchange; csrc/mpp_tempering.hip) ------------- */
/* Every chain anneals by its own triple (current T, alpha, T_target) in device memory.  sched: HOST [n_chains][3].
 * mpp_get_schedules reads the triples as the last launch left them (the kernels write the current temperature back);
 * mpp_set_schedules replaces them and touches nothing else (no step counter, no ladder): -1 if a triple has T < T_target or
 * an entry that is not finite, and then nothing is written.  mpp_set_schedule gives every chain the same triple, resets the
 * step counters as before, and clears any ladder. */
int mpp_get_schedules(mpp_ctx *ctx, double *sched);
int mpp_set_schedules(mpp_ctx *ctx, const double *sched);
/* The temperature ladder over the "replicas" R >= 2 chains of every tile; call it after mpp_set_schedule(T0, alpha, T_target).
 * Chain r * n + i (n tiles) is replica r of tile i and gets (T0 * f_r, alpha, T_target * f_r) with f_0 = 1.0 and
 * f_r = f_{r-1} * ratio, multiplied one after another in float64; rung[r * n + i] = r; the exchange counters (the options
 * below) are zeroed.  A rung is a place on the ladder: an accepted exchange swaps the schedule triples and the rungs of two
 * chains, so the chain at rung 0 of a tile is the one that currently follows the coldest schedule.
 * -1 with a message: no maps, R < 2, a ratio < 1 or not finite.  Cleared by mpp_set_schedule and mpp_set_maps. */
int mpp_set_ladder(mpp_ctx *ctx, double ratio);
/* One attempted exchange: at absolute step `step`, tile `tile`, between rung k (chain_a, energy Ea, current temperature Ta)
 * and rung k + 1 (chain_b, Eb, Tb) -- chain indices of the ctx, all values as read BEFORE the swap; u the uniform draw. */
typedef struct { int64_t step; int32_t tile, k, chain_a, chain_b, accepted, _pad; double Ea, Eb, Ta, Tb, u; } mpp_exchange_record;
/* mpp_run(ctx, n_steps, seed, chain0, -1, NULL, NULL) with an exchange whenever the chains reach an absolute step count
 * s > 0 with s % every == 0 (s as mpp_step_index reports it: cutting a run into calls changes neither the chains nor the
 * log).  The exchange at s, e = s / every, entirely on the ctx's stream -- no energy, temperature or decision reaches the host:
 *   1. every chain's energy, by the launches of mpp_total_energy_all (the same bits);
 *   2. one kernel, one thread per (tile i, pair (k, k + 1)), k + 1 < R: for R = 2 the only pair at every exchange, for R > 2 the
 *      pairs with k % 2 == e % 2.  a / b: the chains of tile i at rungs k / k + 1.
 *        d = (1.0 / Ta - 1.0 / Tb) * (Ea - Eb)                                     (float64)
 *        u = u53(w[0], w[1]), w = Philox4x32-10(ctr = (lo32(s), hi32(s), 0x80000000 | k, chain id), key = seed), chain id and
 *            seed those of replica 0 of tile i: its mpp_set_chain_keys entry when keys are in force, else (chain0 + i, seed).
 *            The chains' own draws use blocks 0..2 and the split / merge ones; the high bit keeps this draw apart;
 *        accept iff Ta > 0, Tb > 0, Ea and Eb finite, and (d >= 0 or u < exp(d)).
 *      On accept the two schedule triples and the two rungs are swapped; points, keys, intensity and step stay.
 * The log (HOST, log_cap records, may be NULL) receives the call's records ordered by (exchange, tile, pair); records past
 * log_cap are dropped and still counted in *n_logged_or_null.  mpp_last_kernel_ms: the sum over the segments.
 * -1 with a message: no ladder; every < 1; the chains of the ctx are not all at the same step.  A sticky chain error ends the
 * call before the next exchange with that error's code.
 * Read-only options, zeroed by mpp_set_ladder: "tempering_exchanges" (exchange steps so far), "tempering_attempts" and
 * "tempering_accepted" (pairs), "tempering_ms" / "tempering_us" (time of the energy and exchange launches, from events,
 * rounded to whole milliseconds / microseconds). */
int mpp_run_tempered(mpp_ctx *ctx, int64_t n_steps, uint64_t seed, uint32_t chain0, int64_t every,
                     mpp_exchange_record *log_or_null, int64_t log_cap, int64_t *n_logged_or_null);

/* score-map epilogue of the two U-Nets (position_net/pos_net_model.py:186-200,338-346,
 * torch_div.py:8-43; shape_net/shape_net_model.py:139-141): all device pointers.
 * pos_out: [3][ldh][ldw] (vec0, vec1, mask logit; the padded output, whose top-left H x W region, the crop, is used) -> det;
 * logits: [32][ldh][ldw] of one mark head -> marks [..][32] (16-byte aligned), softmax over the 32 classes.
 * Every epilogue has one entry point, a window form, for a forward that walks a large image in crops: H x W is the crop's
 * extent (it decides where the divergence is one-sided), (wx0, wy0, wh x ww) the window in crop coordinates; det / marks point
 * to the window's first pixel in a map whose rows are ld_det / ld_marks pixels apart.  The whole crop is the window
 * (0, 0, H x W), into a dense map with ld = W.  A pixel's result does not depend on the window, bit for bit; nothing outside it
 * is written.  A window outside the crop or ld < ww: -1 and a message. */
int mpp_posnet_epilogue_win(mpp_ctx *ctx, int H, int W, int ldh, int ldw, const float *pos_out, double div_w, double div_b,
                            int wx0, int wy0, int wh, int ww, float *det, int ld_det);
int mpp_shapenet_epilogue_win(mpp_ctx *ctx, int H, int W, int ldh, int ldw, const float *logits, int wx0, int wy0, int wh, int ww,
                              float *marks, int ld_marks);
/* epilogue of one convolution of a DoubleConv block (model_parts/unet/unet_parts.py:12-31), in place on the
 * convolution's output x [planes][hw] (NCHW, plane p = channel p % C; float32 or bfloat16, device pointers):
 * x <- max(0, x * scale[c] + shift[c]) with scale = gamma / sqrt(var + eps) and
 * shift = beta + (conv_bias - mean) * scale, i.e. bias + BatchNorm(eval) + ReLU in one pass. */
int mpp_affine_relu(mpp_ctx *ctx, void *x, int planes, int C, int64_t hw, int elem_bytes, const float *scale,
                    const float *shift);

/* The two epilogues above on channels-last network outputs: pos_out [ldh][ldw][3], logits [ldh][ldw][32], elements
 * float32 (elem_bytes 4) or bfloat16 (2), device pointers; same arithmetic, windows and outputs (det, marks float32).  A
 * pixel's 32 logits are contiguous here, so the softmax is one coalesced pass with no transpose. */
int mpp_posnet_epilogue_nhwc_win(mpp_ctx *ctx, int H, int W, int ldh, int ldw, const void *pos_out, int elem_bytes, double div_w,
                                 double div_b, int wx0, int wy0, int wh, int ww, float *det, int ld_det);
int mpp_shapenet_epilogue_nhwc_win(mpp_ctx *ctx, int H, int W, int ldh, int ldw, const void *logits, int elem_bytes, int wx0, int wy0,
                                   int wh, int ww, float *marks, int ld_marks);

/* Channels-last (NHWC) glue between two convolutions of the U-Nets, ONE pass over the activation (device pointers,
 * float32 or bfloat16 elements; in_bytes / out_bytes = 4 or 2):
 *   y [H+2*pad][W+2*pad][C0+C1] <- reflect_pad( f( maxpool2x2( cat(x0 [..][C0], x1 [..][C1]) ) ) )
 * with f(v) = max(0, v*scale[c] + shift[c]) (bias + BatchNorm(eval) + ReLU folded as in mpp_affine_relu; identity when
 * scale == shift == NULL), pool != 0: the sources are [2H][2W] and are max-pooled 2x2 (after f), C1 == 0: no concat,
 * pad = 0 or 1 (reflect, the padding_mode of every 3x3 convolution).  Replaces F.pad(mode="reflect") + BatchNorm2d +
 * ReLU (model_parts/unet/unet_parts.py:12-31), MaxPool2d(2) (:34-45) and torch.cat([skip, up]) (:48-67).
 * y == x0 is allowed when pad == pool == C1 == 0 (in-place epilogue). */
int mpp_nhwc_glue(mpp_ctx *ctx, const void *x0, const void *x1, void *y, int H, int W, int C0, int C1, int pad, int pool,
                  int in_bytes, int out_bytes, const float *scale, const float *shift);

/* One Conv2d(C_in -> 32, kernel 3, padding 1, padding_mode='reflect') of a DoubleConv (model_parts/unet/unet_parts.py:12-31)
 * on the matrix cores (v_mfma_f32_32x32x2_f32: float32 in, float32 accumulate), for the U-Nets' full-resolution level where
 * the library's N = 32 kernels are slowest: x0 [H][W][32] float32 channels-last; x1 = NULL, or the second half of the
 * concatenation cat([skip, up]) of `Up` (unet_parts.py:48-67) as a second [H][W][32] source (C_in = 64, no concatenated
 * copy); wp [C_in / 32][3*3][32 in][32 out] = weight[o][32 s + i][kh][kw] repacked; in_scale / in_shift [32] (or both NULL):
 * x0 <- max(0, x0 * in_scale + in_shift) at the load, i.e. the BatchNorm + ReLU of the layer that produced x0;
 * y [H][W][32] <- (relu ? max(0, .) : .)(conv * out_scale + out_shift) with this layer's folded bias + BatchNorm (or both
 * NULL).  Reflect padding is index arithmetic (no padded copy).  All device pointers, the ctx's stream. */
int mpp_conv3x3_c32(mpp_ctx *ctx, const float *x0, const float *x1, int H, int W, const float *wp, const float *in_scale,
                    const float *in_shift, const float *out_scale, const float *out_shift, int relu, float *y);

/* The stem of a U-Net: Conv2d(3 -> 32, 3x3, padding_mode='reflect') + folded bias / BatchNorm + ReLU
 * (model_parts/unet/unet_parts.py:12-31, first convolution of the first DoubleConv): x [H][W][3] float32 channels-last ->
 * y [H][W][32] = max(0, conv * scale + shift); wp [9 taps][3 in][32 out].  Device pointers, the ctx's stream. */
int mpp_conv3x3_stem(mpp_ctx *ctx, const float *x, int H, int W, const float *wp, const float *scale, const float *shift, float *y);

/* ShapeNet's three 1x1 heads, their biases and the softmax in one pass (model_parts/shape_net.py:12-46,
 * shape_net_model.py's inference softmax): h [ldh][ldw][32] float32 channels-last (the backbone's output) ->
 * marks_* [..][32] = softmax_c(sum_i w[k][c][i] * h[i] + b[k][c]), k = size, ratio, angle; w [3][32 classes][32 in],
 * b [3][32].  Replaces three library convolutions + bias adds + mpp_shapenet_epilogue_nhwc_win (same values up to float32
 * summation order).  All device pointers, 16-byte aligned; the ctx's stream.  The window (wx0, wy0, wh x ww) of the H x W crop
 * and the three destinations' common row pitch ld_marks are those of the epilogues above. */
int mpp_shapenet_heads_win(mpp_ctx *ctx, int H, int W, int ldh, int ldw, const float *h, const float *w, const float *b, int wx0, int wy0,
                           int wh, int ww, float *marks_size, float *marks_ratio, float *marks_angle, int ld_marks);

/* IoU matrix of convex quadrilaterals for the DOTA task-1 evaluation: a [n][8], b [m][8] (x1 y1 .. x4 y4, either
 * orientation) -> out [n][m] = |A_i n B_j| / (|A_i| + |B_j| - |A_i n B_j|), or -1 where the axis-aligned extents
 * (inclusive-pixel +1 convention) do not overlap.  Stands in for `polyiou.iou_poly` and the hbb pre-filter of
 * DOTA_devkit dota_evaluation_task1.voc_eval as called from metrics/dota_eval.py:37-47 (devkit not vendored,
 * README.md:22-30).  on_device != 0: a, b, out are device pointers. */
int mpp_quad_iou(mpp_ctx *ctx, int n, const double *a, int m, const double *b, double *out, int on_device);

/* The CNN-only baseline's detection step (csrc/mpp_detect.hip): the PosNet / ShapeNet inference of
 * position_net/pos_net_model.py:376-380 and shape_net/shape_net_model.py:283-288 (and naive_detection,
 * sample_rjmcmc.py:23-27) on a whole score map.  det [H][ld] float32, xy [cap][2] int32 (row, col) and scores [cap] float32
 * are device pointers; n_candidates / n_kept are host pointers; the ctx's stream, synchronous up to the last kernel.
 *  - candidates: det > (float)threshold when strict (PosNet), det >= (float)threshold otherwise (ShapeNet's PosNet call,
 *    naive_detection) -- a float32 compare against the threshold rounded to float32, as NumPy compares a float32 array
 *    with a Python float (mpp_naive_init's compare is the same one);
 *  - rank: value descending, ties toward the larger row-major flat index r*W + c (-0 ties with +0);
 *  - NMS: in rank order a candidate is kept iff every kept candidate ranked above it lies at sqrt(dx^2+dy^2) > nms_distance
 *    (double; utils/nms.py:68-110), 0 <= nms_distance <= 32 (else -1);
 *  - output: the kept centres and their scores in pick (rank) order.  No cap of its own: if more than cap are kept it
 *    returns -13, *n_kept = the number needed, and writes nothing to xy / scores.  H*W >= 2^31: -1.
 * Read-only option "detect_launches": the resolve launches of the last call.  -9: a resolve that stopped making progress. */
int mpp_detect_centers(mpp_ctx *ctx, int H, int W, int ld, const float *det, double threshold, int strict, double nms_distance,
                       int cap, int32_t *xy, float *scores, int64_t *n_candidates, int64_t *n_kept);
/* The argmax class of each of the three mark maps m0..m2 [H][ld][32] float32 (first maximum, a NaN wins: np.argmax) at the
 * n pixels xy [n][2] (row, col): classes [n][3] int32, -1 for a pixel outside the map -- output_vector_to_value
 * (shape_net/mappings.py:145-157) at ShapeNet's centres.  All device pointers, the ctx's stream (asynchronous). */
int mpp_mark_classes(mpp_ctx *ctx, int H, int W, int ld, const float *m0, const float *m1, const float *m2, int n,
                     const int32_t *xy, int32_t *classes);

/* ---- training the U-Nets (csrc/mpp_train.hip) ------------------------------------------------------------------------
 * The training images of a dataset, resident on the device: images uint8 [H][W][3] back to back (img_off[i] bytes from
 * images, img_hw[i] = {H, W}); the objects of image i are rows obj_start[i] .. obj_start[i+1]-1 of centers [n][2] int32
 * (row, col) and params [n][3] float64 (a, b, angle), in annotation order.  All device pointers. */
typedef struct mpp_train_data {
  const uint8_t *images;
  const int64_t *img_off;
  const int32_t *img_hw;
  const int32_t *obj_start;
  const int32_t *centers;
  const double *params;
  int32_t n_images;
  int32_t _pad;
} mpp_train_data;
/* What the labels are made of.  kind 0: PosNet (models/position_net/data_loaders.py:23-118, target uvec or vec, a numeric
 * max_distance, sigma_dil); kind 1: ShapeNet (models/shape_net/data_loaders.py:41-118, mask_mode shapes) with the three
 * value mappings: n_classes <= 32 lower bin edges per mark, cyclic[k] for the angle. */
typedef struct mpp_train_labels {
  int32_t kind;
  int32_t uvec;
  double max_distance;
  double sigma_dil;
  int32_t n_classes;
  int32_t cyclic[3];
  double edges[3][MPP_NCLASS];
} mpp_train_labels;
/* Outputs of mpp_train_batch, device pointers (NULL: not written, except patch and sums).  nb = ceil(P / MPP_TRAIN_BAND).
 *  patch [B][3][P][P] float32 (value / 255);
 *  PosNet: vec [B][2][P][P], mask [B][P][P], dil (center_binary_map_dil) [B][P][P], dist (distance to the nearest centre)
 *  [B][P][P], all float32;  ShapeNet: cls [3][B][P][P] uint8 (value_class_map), cover [B][P][P] uint8 (the union of the
 *  object masks; loss_mask = cover / sum of the patch's cover);
 *  sums [B][nb][2] float64: per row band of a patch, the count of mask (PosNet) or cover (ShapeNet) pixels and the sum of
 *  dil (PosNet);  status [1] int32: the largest object count of a patch that exceeded MPP_TRAIN_MAX_OBJ (0: none). */
typedef struct mpp_train_out {
  float *patch;
  float *vec;
  float *mask;
  float *dil;
  float *dist;
  uint8_t *cls;
  uint8_t *cover;
  double *sums;
  int32_t *status;
} mpp_train_out;
#define MPP_TRAIN_BAND 16          /* rows of a patch per workgroup of mpp_train_batch */
#define MPP_TRAIN_MAX_OBJ 1024     /* objects of one patch held in LDS */
#define MPP_TRAIN_MAX_P 1024
enum {
  MPP_AUG_GEOMETRIC = 1,           /* D4: rotation by k*90 deg (p 0.5), then a vertical / horizontal / both flip (p 0.5) */
  MPP_AUG_MEDIUM = 2,              /* photometric part of data/augmentation.py:22-40 that is one formula per op */
  MPP_AUG_STRONG = 4,              /* ... of :43-72 */
  MPP_AUG_PERTURB = 8,             /* ShapeNet: class perturbation {0: 0.8, +1: 0.1, -1: 0.1} per object and mark */
  MPP_AUG_HISTMATCH = 16,          /* histogram matching to a random image of the subset (p 0.5), blended with U(0.1, 0.75);
                                      needs mpp_train_set_histograms */
  MPP_AUG_SPATIAL = 32             /* the ops of the recipe that need neighbours or the whole patch: shadow, fog, CLAHE,
                                      downscale, median / box blur (below); needs P % 8 == 0 and 32 <= P <= 512 */
};
/* One batch of B patches of P x P (P even, 8..MPP_TRAIN_MAX_P) from the resident images: desc [B][3] int32 = (image, anchor
 * row, anchor col) device array; the patch is the read at anchor - P/2 with zeros outside the image (utils/images.py:4-23),
 * its objects those with anchor - P/2 <= centre < anchor - P/2 + P (data/patch_dataset.py:41-89).  flags: MPP_AUG_*.  Every
 * random draw is Philox4x32-10 with key (seed, epoch) and counter (batch, patch, stream, index): the same arguments give
 * the same batch bit for bit.  One launch on the ctx's stream (asynchronous).  -1: bad arguments. */
int mpp_train_batch(mpp_ctx *ctx, const mpp_train_data *data, const mpp_train_labels *labels, int B, int P,
                    const int32_t *desc, int flags, uint32_t seed, uint32_t epoch, uint32_t batch, const mpp_train_out *out);
/* PointingVectorLoss (model_parts/losses/pos_loss.py:36-115; learn_mask, compute_relevant, balanced_mask_loss,
 * vec_loss_on_prod, no focal loss) of out [B][3][P][P] float32 against vec / mask / dil of mpp_train_batch.  with_div 1
 * (training, pos_net_model.py:116-138): also the divergence classifier conv(div(out[:, :2]) * sigmoid(out[:, 2]); w, b)
 * against dil, w and b float32 device scalars.  res [8] float64 (device): vec_loss, mask_loss, div_loss, loss, dL/dw,
 * dL/db; grad [B][3][P][P] float32 = dL/dout (NULL: losses only).  One launch on the ctx's stream (asynchronous). */
int mpp_posnet_loss(mpp_ctx *ctx, int B, int P, const float *out, const float *vec, const float *mask, const float *dil,
                    const double *sums, int with_div, const float *w, const float *b, float *grad, double *res);
/* PixelCELoss (model_parts/losses/pixel_ce_loss.py:20-57, no focal loss) of the three heads l0..l2 [B][n_classes][P][P]
 * float32 against cls / cover / sums of mpp_train_batch: per head the cross-entropy times loss_mask summed over the
 * pixels, averaged over the batch (float64 sums).  res [8] float64 (device): loss_feat0..2, loss; g0..g2 = dL/dlogits
 * (NULL: losses only).  One launch on the ctx's stream (asynchronous). */
int mpp_shapenet_loss(mpp_ctx *ctx, int B, int P, int n_classes, const float *l0, const float *l1, const float *l2,
                      const uint8_t *cls, const uint8_t *cover, const double *sums, float *g0, float *g1, float *g2,
                      double *res);


/* ---- histogram matching and error-density resampling (csrc/mpp_train.hip, csrc/mpp_resample.hip) ---------------------
 * MPP_AUG_HISTMATCH is skimage's match_histograms per channel on the 8-bit values of the P x P crop (its zero padding
 * included) against the full-resolution histogram of a template image of the same subset:
 *   src_q = cumsum(bincount(s)) / s.size;  tmpl_q = cumsum(counts of the template's present values) / t.size;
 *   lut = interp(src_q, tmpl_q, present values) in float64;  out = blend * lut[s] + (1 - blend) * s.
 * It sits after the D4 element and before every other photometric op.  Its three draws are words 0..2 of Philox stream 0,
 * index 5 of the patch: apply (u < 0.5), template = floor(u * n_images), blend = 0.1 + u * 0.65.
 *
 * mpp_image_histograms: hist [n_images][3][256] uint32 (device) of the resident images (each of fewer than 2^32 pixels,
 * at most 65535 images), one launch on the ctx's stream after reading the image sizes back.
 * mpp_train_set_histograms: hands that table (borrowed, device) to the ctx for the following mpp_train_batch calls with
 * MPP_AUG_HISTMATCH; n_images must equal the data's (else mpp_train_batch returns -1); NULL takes it away. */
int mpp_image_histograms(mpp_ctx *ctx, const mpp_train_data *data, uint32_t *hist);
int mpp_train_set_histograms(mpp_ctx *ctx, const uint32_t *hist, int n_images);
/* The error density of one training image (H x W) from a raw PosNet output: out [3][ldh][ldw] float32 is the forward of
 * the crop whose pixel (0, 0) is image pixel (cx0, cy0); the cells of the core (x0, x1, y0, y1) -- image rows x0..x1-1,
 * columns y0..y1-1; x0 and y0 multiples of 8, x1 (y1) a multiple of 8 or H (W) -- are written.  With
 *   target = 1 where the nearest of the n centres [n][2] int32 (row, col; image coordinates) is within max_distance
 *            (the `mask` label of mpp_train_batch; 0 without objects),
 *   err = |target - sigmoid(out[2])| in float32,  cell = mean of err over the in-image pixels of an 8 x 8 block,
 * dens [ceil(H/8)][ceil(W/8)] uint8 = min(255, floor(256 * cell)); *sum (uint64, device) grows by the sum of the cells
 * written (zero it before the first core of an image); cell_out (NULL-able) the float32 means.  n is not limited.
 * All device pointers, one launch on the ctx's stream (asynchronous). */
int mpp_posnet_error_map(mpp_ctx *ctx, int H, int W, int ldh, int ldw, const float *out, int cx0, int cy0, int x0, int x1,
                         int y0, int y1, const int32_t *centers, int n, double max_distance, uint8_t *dens,
                         unsigned long long *sum, float *cell_out);
/* Integer prefix tables of the densities of n_images images (img_hw [n_images][2] int32 as in mpp_train_data), cell maps
 * back to back: image i's [ceil(H/8)][ceil(W/8)] map starts cell_off[i] entries into dens / cellcum, its rows row_off[i]
 * entries into rowcum (total_rows = row_off past the last image).  cellcum: inclusive prefix within each row (uint32);
 * rowcum: inclusive prefix of the row totals (uint64), so the image's total is its last entry. */
int mpp_density_prefix(mpp_ctx *ctx, int n_images, const int32_t *img_hw, const int64_t *cell_off, const int64_t *row_off,
                       int64_t total_rows, const uint8_t *dens, uint32_t *cellcum, unsigned long long *rowcum);
/* n anchors from those tables: rows [n][2] int32 = (image, plan row).  w = Philox4x32-10 words (1 << 32 | 0) with key
 * (seed, epoch) and counter (plan row, 0, 3, 0); r = mulhi64(w, total); (I, J) the cell whose cumulative range holds r;
 * anchors [n][2] int32 = (min(8 I, H), min(8 J, W)), or (-1, -1) for an image whose total is 0. */
int mpp_density_anchors(mpp_ctx *ctx, int n_images, const int32_t *img_hw, const int64_t *cell_off, const int64_t *row_off,
                        const uint32_t *cellcum, const unsigned long long *rowcum, int n, const int32_t *rows,
                        uint32_t seed, uint32_t epoch, int32_t *anchors);

/* ---- the spatial ops of the augmentation recipe (csrc/mpp_train.hip, MPP_AUG_SPATIAL) ----------------------------------
 * With the flag the image of a patch goes through the whole recipe of data/augmentation.py:21-71, in its order:
 *   medium: D4, hist-match, OneOf[CLAHE | RGBShift], OneOf[Median3 | Blur3] (p 0.2), GaussNoise
 *   strong: D4, hist-match, Shadow, Fog, OneOf[Shuffle | Dropout], BrightnessContrast, OneOf[CLAHE | RGBShift | ToGray],
 *           Downscale(0.9), OneOf[Median3 | Blur3] (p 0.2), GaussNoise
 * Labels do not move.  A patch whose draws pick none of the six ops is bit for bit the patch without the flag.  The ops are
 * defined in DESIGN.md section 8; their patch draws are words of Philox stream 0, indices 6 and 7, their lists (shadow
 * vertices, haze points) come from stream 3 (the table is in csrc/mpp_train.hip).
 *
 * mpp_train_aug_params writes what mpp_train_batch with the same (flags, seed, epoch, batch, B, P, n_images) draws for every
 * patch: out [B] mpp_aug_record, device memory, one launch on the ctx's stream (asynchronous).  It reads no image. */
#define MPP_AUG_MAX_HAZE 64        /* haze points of one patch (the fog loop gives at most 51 for P <= 512) */
typedef struct mpp_aug_record {
  int32_t rot, flip;               /* D4 */
  int32_t chan_op, chan_arg;       /* 1 shuffle (permutation chan_arg of 6), 2 dropout (channel chan_arg) */
  int32_t bc;                      /* brightness / contrast applies (alpha, beta) */
  int32_t color;                   /* 1 RGB shift (shift), 2 to gray; 0 with clahe 1: CLAHE */
  int32_t noise;                   /* Gauss noise applies (sigma) */
  int32_t hm, tmpl;                /* histogram matching to image tmpl (blend) */
  int32_t shadow, n_poly;          /* RandomShadow applies with n_poly (1 or 2) polygons of 5 vertices */
  int32_t fog, n_haze;             /* RandomFog applies (fog_coef) with n_haze haze points */
  int32_t clahe;                   /* CLAHE applies (clip) */
  int32_t downscale;               /* Downscale(0.9) applies */
  int32_t blur;                    /* 1 MedianBlur(3), 2 Blur(3) */
  float alpha, beta, shift[3];
  float _pad;
  double sigma, blend, clip, fog_coef;
  int16_t poly[2][5][2];           /* (x, y) = (column, row) of the shadow vertices, in the order drawn */
  int16_t haze[MPP_AUG_MAX_HAZE][2];   /* (x, y) of the haze points, in the order drawn */
} mpp_aug_record;
int mpp_train_aug_params(mpp_ctx *ctx, int flags, uint32_t seed, uint32_t epoch, uint32_t batch, int B, int P, int n_images,
                         mpp_aug_record *out);

/* ---- dataset translation: the anti-aliased rescale (csrc/mpp_rescale.hip) ------------------------------------------------
 * What data/translation/translate_DOTA.py:181 and translate_COWC.py:52 compute per image, skimage 0.18.1
 * rescale(image / 255, scale, anti_aliasing=True, multichannel=True) followed by plt.imsave, as a generic separable
 * resampler.  The caller folds the Gaussian blur (mirror boundary) and the bilinear interpolation of each axis into a table
 * of (source index, weight) pairs per output row and per output column; then, in float64,
 *   v[i][j][c]   = sum_t row_w[i][t] * ( sum_s col_w[j][s] * src[row_idx[i][t]][col_idx[j][s]][c] / 255 ),  t, s ascending
 *   out[i][j][c] = (uint8)(255 * min(max(v, 0), 1))            -- truncation, as plt.imsave stores it
 * src: uint8 [H][W][3], device, rows src_pitch bytes apart (>= 3 W); row_idx / row_w [oh][row_taps] and col_idx / col_w
 * [ow][col_taps]: HOST arrays, read before the call returns, every index inside the image (checked); out: uint8
 * [oh][ow][3], device, contiguous; out_f64 (NULL-able): v, float64 [oh][ow][3], device.  H * W * 3 may reach 2^31.
 * The horizontally filtered rows are kept in a workspace of the ctx (grown on demand) for one band of output rows at a
 * time; tables plus band stay within workspace_limit bytes (too small for one output row: an error), and neither out nor
 * out_f64 depends on the bands.  Option rescale_bands: the bands of the last call.  Launches on the ctx's stream,
 * asynchronous. */
int mpp_rescale(mpp_ctx *ctx, const uint8_t *src, int H, int W, int64_t src_pitch, const int32_t *row_idx,
                const double *row_w, int oh, int row_taps, const int32_t *col_idx, const double *col_w, int ow, int col_taps,
                uint8_t *out, double *out_f64, int64_t workspace_limit);

/* ---- the result pictures of infer (csrc/mpp_figures.hip) ---------------------------------------------------------------------
 * What models/shape_net/display.py:37-59 draws with OpenCV -- rectangle outlines over the picture -- as RGB8 [H][W][3]
 * (device, contiguous), composed where the picture and the score maps already are.  DESIGN.md section 11 has the rules:
 *   base     rgb: float32 [H][W][3] in 0..1 (device), or scalar: float32 [H][W] (device) clipped to [vmin, vmax] and looked
 *            up in lut, float32 [256][3] (host), at min(255, (int)((v - vmin) / (vmax - vmin) * 256)) in float64; exactly
 *            one of rgb and scalar is given;
 *   outline  corners: int32 [n][4][2] (host), (row, col) per corner, |coordinate| <= 2^20; edge k of a rectangle is the integer
 *            8-connected Bresenham walk from corner k to corner (k + 1) % 4; pixels outside the image are skipped;
 *   order    a pixel on several outlines takes the colour of the rectangle with the highest index, as drawing them one
 *            after another does; colors: float32 [n][3] (host);
 *   8 bits   (uint8)(v * 255) in float32, truncated, as matplotlib's imsave; a pixel with a NaN channel is (0, 0, 0).
 * n = 0 gives the base picture.  Runs on the ctx's stream and returns when the picture is complete: the host tables are the
 * caller's again. */
int mpp_draw_outlines(mpp_ctx *ctx, int H, int W, const float *rgb, const float *scalar, double vmin, double vmax,
                      const float *lut, int n, const int32_t *corners, const float *colors, uint8_t *out);

void mpp_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
int mpp_abi_version(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
