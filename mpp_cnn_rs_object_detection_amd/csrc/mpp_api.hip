// mpp_api.hip -- host side of the C ABI declared in include/mpp_hip.h: the life cycle of a context, its options, what it is
// given (model, kernels, maps, image), the per-tile pointer table and point I/O.  Chains: mpp_api_chain.hip; from-scratch
// energies: mpp_api_energy.hip; U-Nets and training: mpp_api_nets.hip; the context they share: mpp_ctx.hpp.
#include "mpp_ctx.hpp"
#include "mpp_window.hpp"

// 2: ten kernels (split, merge), mpp_kernels.split_*; 3: mpp_nhwc_glue, mpp_*_epilogue_nhwc; 4: mpp_pack_detections; 5: mpp_set_chain_keys, options auto_grow / remap_table
extern "C" int mpp_abi_version(void) { return 10; }

extern "C" void mpp_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}

extern "C" int mpp_create(int device_id, mpp_ctx **out) {
  if (!out) return -1;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return -3;   // no GPU: fail loudly, no CPU fallback
  if (device_id < 0 || device_id >= count) return -1;
  mpp_ctx *c = new mpp_ctx();
  c->device = device_id;
  memset(&c->hp, 0, sizeof(DevParams));
  c->hp.n_kernels = MPP_K_SPLIT;
  c->hp.hot_past = 1;
  if (hipSetDevice(device_id) != hipSuccess || hipStreamCreate(&c->own_stream) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
      hipEventCreate(&c->ev2) != hipSuccess || hipEventCreate(&c->ev3) != hipSuccess ||
      c->dp.alloc(1) != hipSuccess) {
    delete c;
    return -2;
  }
  c->stream = c->own_stream;
  *out = c;
  return 0;
}

static void free_tiles(mpp_ctx *c) {
  if (!c->maps_borrowed) {
    if (c->det) (void)hipFree(c->det);
    for (int k = 0; k < 3; ++k) if (c->m[k]) (void)hipFree(c->m[k]);
  }
  c->det = nullptr; c->m[0] = c->m[1] = c->m[2] = nullptr;
  if (c->img && !c->img_borrowed) (void)hipFree(c->img);
  c->img = nullptr; c->img_c = 0; c->img_borrowed = false;
  static_cast<TileMem &>(*c) = TileMem();
  c->remap_dirty = true;
}

extern "C" int mpp_destroy(mpp_ctx *c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  free_tiles(c);
  mpp_detect_free(&c->detect);
  mpp_train_ws_free(&c->train);
  mpp_rescale_ws_free(&c->rescale);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev2) (void)hipEventDestroy(c->ev2);
  if (c->ev3) (void)hipEventDestroy(c->ev3);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;                                      // (the workspaces and the parameter block go with their owners)
  return 0;
}

extern "C" const char *mpp_last_error(mpp_ctx *c) { return c ? c->err.c_str() : "no context"; }

extern "C" int mpp_set_stream(mpp_ctx *c, void *s) {
  if (!c) return -1;
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return 0;
}
extern "C" int mpp_synchronize(mpp_ctx *c) {
  if (!c) return -1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int mpp_set_option(mpp_ctx *c, const char *name, int64_t v) {
  if (!c || !name) return -1;
  if (!strcmp(name, "spec_waves")) {
    if (v != 1 && v != 2 && v != 4 && v != 8 && v != 16) return fail(c, -1, "spec_waves must be 1, 2, 4, 8 or 16");
    c->spec = (int)v;
  } else if (!strcmp(name, "spec_lanes")) {
    // lane mode: 4 waves, `v` lanes of each evaluate one speculative step each (4*v steps per round); 0 = off
    if (v != 0 && v != 1 && v != 2 && v != 4 && v != 8 && v != 16) return fail(c, -1, "spec_lanes must be 0, 1, 2, 4, 8 or 16");
    c->lanes = (int)v;
  } else if (!strcmp(name, "deep")) {
    if (v != 0 && (v < 8 || v > 256 || (v & (v - 1)))) return fail(c, -1, "deep must be 0 or a power of two in 8..256");
    c->deep = (int)v;
  } else if (!strcmp(name, "handover")) {
    if (v != 0 && v != 1) return fail(c, -1, "handover must be 0 or 1");
    c->handover = (int)v;
  } else if (!strcmp(name, "handover_at")) {
    if (v < 256 || v > 2048) return fail(c, -1, "handover_at must be in 256..2048 (steps committed per round of 8, x 256)");
    c->handover_at = (int)v;
  } else if (!strcmp(name, "handover_tiles")) {
    if (v < 1 || v > 65536) return fail(c, -1, "handover_tiles must be in 1..65536");
    c->handover_tiles = (int)v;
  } else if (!strcmp(name, "deep_gain")) {
    if ((v & 0xff) < 8 || (v & 0xff) > 64 || (v & ~0x1ffll)) return fail(c, -1, "deep_gain must be in 8..64 (eighths; + 256: sorted steps dealt in blocks)");
    c->deep_gain = (int)v;
  } else if (!strcmp(name, "deep_fixed")) {
    if (v < 0 || v > 256) return fail(c, -1, "deep_fixed must be in 0..256");
    c->deep_fixed = (int)v;
  } else if (!strcmp(name, "replicas")) {
    // independent replica chains per tile: mpp_set_maps(n_tiles = M) then creates M*v chains, chain t on the maps
    // of tile t % M (several chains of one tile with different chain ids, or a benchmark's many-tile load)
    if (c->have_maps) return fail(c, -1, "replicas must be set before mpp_set_maps");
    if (v < 1 || v > 65536) return fail(c, -1, "replicas out of range");
    c->replicas = (int)v;
  } else if (!strcmp(name, "point_capacity")) {
    if (c->have_maps) return fail(c, -1, "point_capacity must be set before mpp_set_maps");
    if (v < 1 || v > 65535) return fail(c, -1, "point_capacity out of range");
    c->cap = (int)v;
  } else if (!strcmp(name, "scratch_grid_min_points")) {
    // configurations of at least this many points get a candidate grid for the from-scratch energies; 0 = never
    if (v < 0) return fail(c, -1, "scratch_grid_min_points must be >= 0");
    c->grid_min_points = (int)v;
  } else if (!strcmp(name, "recombine_lds_points")) {
    // mpp_recombine labels a tile of at most this many points (over its replicas) in LDS, a larger one in device memory
    if (v < 0 || v > MPP_RECOMBINE_LDS_POINTS) return fail(c, -1, "recombine_lds_points must be in 0..%d", MPP_RECOMBINE_LDS_POINTS);
    c->recombine_lds = (int)v;
  } else if (!strcmp(name, "cell_capacity")) {
    if (v < 1 || v > MPP_CELL_CAP_MAX) return fail(c, -1, "cell_capacity must be in 1..%d", MPP_CELL_CAP_MAX);
    c->cell_cap = (int)v; c->params_dirty = true;
  } else if (!strcmp(name, "auto_grow")) {
    c->auto_grow = v ? 1 : 0;
  } else if (!strcmp(name, "chain_state")) {
    if (v < 0 || v > 2) return fail(c, -1, "chain_state must be 0 (auto), 1 (LDS only) or 2 (device memory for every chain)");
    c->chain_state = (int)v;
  } else if (!strcmp(name, "remap_table")) {
    if (v < -1 || v > 1) return fail(c, -1, "remap_table must be -1 (auto), 0 or 1");
    c->remap_mode = (int)v; c->remap_dirty = true;
  } else if (!strcmp(name, "force_accept")) {
    c->hp.force_accept = v ? 1 : 0; c->params_dirty = true;
  } else if (!strcmp(name, "prepass")) {
    if (v < 0 || v > 1) return fail(c, -1, "prepass must be 0 or 1");
    c->prepass = (int)v;
  } else if (!strcmp(name, "prepass_mb")) {
    // (at most 16 GB: a birth's ordinal has 28 bits of its step word)
    if (v < 1 || v > 16384) return fail(c, -1, "prepass_mb must be in 1..16384");
    c->prepass_mb = (int)v;
  } else if (!strcmp(name, "prepass_queues")) {
    if (v < 0 || v > 1) return fail(c, -1, "prepass_queues must be 0 or 1");
    c->prepass_queues = (int)v;
  } else if (!strcmp(name, "hot_table")) {
    if (v < 0 || v > 1) return fail(c, -1, "hot_table must be 0 or 1");
    c->hot_table = (int)v;
  } else if (!strcmp(name, "hot_past_births")) {
    // the table form of the hot start keeps committing a round's steps past an accepted birth / death (0: the round ends there)
    if (v < 0 || v > 1) return fail(c, -1, "hot_past_births must be 0 or 1");
    c->hp.hot_past = (int)v; c->params_dirty = true;
  } else if (!strcmp(name, "window_rows")) {
    // the data-driven translation reads its window's row sums from the transposed table (0: it forms them from rowpart)
    if (v < 0 || v > 1) return fail(c, -1, "window_rows must be 0 or 1");
    c->window_rows = (int)v; c->tiles_dirty = true;
  } else if (!strcmp(name, "deep_skip_same")) {
    // an untraced deep round skips the evaluation of a step that re-writes its target with the values it holds (0: it evaluates it)
    if (v < 0 || v > 1) return fail(c, -1, "deep_skip_same must be 0 or 1");
    c->deep_skip_same = (int)v;
  } else if (!strcmp(name, "deep_carry")) {
    // an untraced queue round keeps the reports behind its end that stay trustworthy; the next round does not evaluate them (0: it does)
    if (v < 0 || v > 1) return fail(c, -1, "deep_carry must be 0 or 1");
    c->deep_carry = (int)v;
  } else return fail(c, -1, "unknown option %s", name);
  return 0;
}
extern "C" int64_t mpp_get_option(mpp_ctx *c, const char *name) {
  if (!c || !name) return -1;
  if (!strcmp(name, "spec_waves")) return c->spec;
  if (!strcmp(name, "spec_lanes")) return c->lanes;
  if (!strcmp(name, "deep")) return c->deep;
  if (!strcmp(name, "deep_fixed")) return c->deep_fixed;
  if (!strncmp(name, "deep_stat", 9) && name[9] >= '0' && name[9] <= '9') {      // deep_stat0 .. deep_stat255 (4 counters, then the per-wave phase clocks of the diagnostic build)
    const int i = atoi(name + 9);
    unsigned long long v[256] = {0};
    if (i > 255) return -1;
    if (c->deep_stats.p && hipMemcpy(v, c->deep_stats.p, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v[i];
  }
  if (!strcmp(name, "point_capacity")) return c->cap;
  if (!strcmp(name, "replicas")) return c->replicas;
  if (!strcmp(name, "n_chains")) return c->n_tiles;
  if (!strcmp(name, "cell_capacity")) return c->cell_cap;
  if (!strcmp(name, "handover")) return c->handover;
  if (!strcmp(name, "handover_tiles")) return c->handover_tiles;
  if (!strcmp(name, "handover_at")) return c->handover_at;
  if (!strcmp(name, "auto_grow")) return c->auto_grow;
  if (!strcmp(name, "remap_table")) return c->remap[0] ? 1 : 0;       // are the tables in use right now?
  if (!strcmp(name, "grow_events")) return c->grow_events;
  if (!strcmp(name, "chain_state")) return c->chain_state;
  if (!strcmp(name, "hbm_chains")) return c->hbm_chains;
  if (!strcmp(name, "hbm_bytes")) return (int64_t)c->hbm_ws.bytes;
  if (!strcmp(name, "prepass")) return c->prepass;
  if (!strcmp(name, "prepass_mb")) return c->prepass_mb;
  if (!strcmp(name, "prepass_used")) return c->prepass_used;
  if (!strcmp(name, "prepass_queues")) return c->prepass_queues;
  if (!strcmp(name, "prepass_queues_used")) return c->prepass_queues_used;
  if (!strcmp(name, "hot_table")) return c->hot_table;
  if (!strcmp(name, "hot_table_used")) return c->hot_table_used;
  if (!strcmp(name, "hot_past_births")) return c->hp.hot_past;
  if (!strcmp(name, "window_rows")) return c->window_rows;
  if (!strcmp(name, "deep_skip_same")) return c->deep_skip_same;
  if (!strcmp(name, "deep_carry")) return c->deep_carry;
  // parallel tempering since the last mpp_set_ladder: exchange steps, attempted and accepted pairs, time of their launches
  if (!strcmp(name, "tempering_exchanges")) return c->x_exchanges;
  if (!strcmp(name, "tempering_attempts")) return c->x_attempts;
  if (!strcmp(name, "tempering_accepted")) {
    if (!c->ladder || !c->x_acc.p) return 0;
    std::vector<long long> acc((size_t)c->n_maps * (c->replicas - 1));
    if (hipMemcpy(acc.data(), c->x_acc.p, acc.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    long long sum = 0;
    for (long long v : acc) sum += v;
    return sum;
  }
  if (!strcmp(name, "tempering_ms")) return (int64_t)llround(c->x_ms);
  if (!strcmp(name, "tempering_us")) return (int64_t)llround(c->x_ms * 1000.0);
  if (!strcmp(name, "detect_launches")) return c->detect.launches;
  if (!strcmp(name, "rescale_bands")) return c->rescale.bands;                  // bands of the last mpp_rescale
  if (!strcmp(name, "rescale_bytes")) return (int64_t)c->rescale.dev_bytes;     // its device workspace right now
  if (!strcmp(name, "scratch_grid_min_points")) return c->grid_min_points;
  if (!strcmp(name, "recombine_lds_points")) return c->recombine_lds;
  if (!strcmp(name, "birth_map_grid")) return c->birth_grid;                    // the last birth map's pre-pass built grids
  if (!strcmp(name, "move_gains_grid")) return c->move_grid;                    // the last move-gain pre-pass built grids
  if (!strcmp(name, "force_accept")) return c->hp.force_accept;
  if (!strcmp(name, "grid_nx")) return c->hp.nx;       // spatial hash dimensions (point_set.py:58-61)
  if (!strcmp(name, "grid_ny")) return c->hp.ny;
  if (!strcmp(name, "grid_res")) return (long long)c->hp.res;
  if (!strcmp(name, "lds_bytes")) {
    // (answers before any launch, so not from hp.rowbase_lds, which run_chain sets per call: its own rule, the row level in LDS
    //  in lane mode only, is narrower than run_chain's; callers size their capacities by the value, so it stays what it was)
    LaunchShape s = launch_shape(c, c->lanes > 0 && c->H <= 1024);
    if (s.ncell <= 0) s.ncell = 1;
    size_t b = chain_lds_total(s, c->cap, c->cell_cap);
    if (c->deep > 0 && c->lanes == 0 && c->spec <= 8) {        // deep rounds: at least the smallest round has to fit
      s.rb_rows = c->H <= 1024 ? c->H + 1 : 0;
      const size_t d = deep_lds_total(s, c->cap, c->cell_cap, 8);
      if (d > b) b = d;
    }
    return (int64_t)b;
  }
  return -1;
}

static void refresh_grid(mpp_ctx *c) {
  DevParams &P = c->hp;
  double maxd = 0.0;
  for (int p = 0; p < P.model.n_pair; ++p) if (P.model.pair[p].max_dist > maxd) maxd = P.model.pair[p].max_dist;
  P.max_inter = P.model.n_pair > 0 ? maxd : 1.0;                  // energy_graph.py:26-29
  P.res = maxd > 32.0 ? maxd : 32.0;                              // point_set.py:7,58
  P.H = c->H; P.W = c->W;
  P.nx = c->H > 0 ? (int)ceil((double)c->H / P.res) : 0;         // point_set.py:59-61
  P.ny = c->W > 0 ? (int)ceil((double)c->W / P.res) : 0;
  P.cap = c->cap; P.cell_cap = c->cell_cap; P.n_tiles = c->n_tiles;
  P.res_int = (int)P.res;
  P.res_shift = -1;
  for (int s = 0; s < 16; ++s) if ((1 << s) == P.res_int) P.res_shift = s;
  for (int p = 0; p < MPP_MAX_PAIR; ++p)
    P.maxd2[p] = p < P.model.n_pair ? (int)floor(P.model.pair[p].max_dist * P.model.pair[p].max_dist + 1e-9) : 0;
  P.conflict_d2 = (int)(4.0 * P.max_inter * P.max_inter) + 1;
  P.uniform_bins = 1;
  for (int k = 0; k < 3; ++k) {
    double range = P.maps.vmax[k] - P.maps.vmin[k];
    P.inv_step[k] = range > 0 ? (double)MPP_NCLASS / range : 0.0;
    for (int i = 0; i < MPP_NCLASS; ++i)
      if (!(fabs(P.maps.edges[k][i] - (P.maps.vmin[k] + range * i / MPP_NCLASS)) <= 1e-9 * (fabs(range) + 1.0)))
        P.uniform_bins = 0;
  }
  c->params_dirty = true;
}

extern "C" int mpp_set_model(mpp_ctx *c, const mpp_model *model, const mpp_mappings *maps) {
  if (!c || !model || !maps) return -1;
  if (model->n_unit < 0 || model->n_unit > MPP_MAX_UNIT || model->n_pair < 0 || model->n_pair > MPP_MAX_PAIR)
    return fail(c, -1, "bad term counts");
  if (model->gate_term >= model->n_unit) return fail(c, -1, "gate_term must index a unit term");
  for (int p = 0; p < model->n_pair; ++p) {
    const mpp_pair_term &t = model->pair[p];
    bool ok = (t.kind == MPP_P_OVERLAP && t.reduce == MPP_REDUCE_MAX) ||
              (t.kind == MPP_P_ALIGN && ((t.p[0] != 0.0) == (t.reduce == MPP_REDUCE_MIN))) ||
              ((t.kind == MPP_P_DIST_LE || t.kind == MPP_P_DIST_LT) && t.reduce == MPP_REDUCE_MAX);
    if (!ok) return fail(c, -1, "pair term %d: unsupported (kind, reduce) combination", p);
    if (!(t.max_dist > 0.0)) return fail(c, -1, "pair term %d: max_dist must be positive", p);
  }
  {
    double maxd = 0.0;
    for (int p = 0; p < model->n_pair; ++p) if (model->pair[p].max_dist > maxd) maxd = model->pair[p].max_dist;
    if (maxd > 32.0 && maxd != floor(maxd))
      return fail(c, -1, "interaction radius %g > 32 must be integral (it is the cell size of the spatial hash)", maxd);
  }
  for (int k = 0; k < 3; ++k)
    for (int i = 1; i < MPP_NCLASS; ++i)
      if (!(maps->edges[k][i] > maps->edges[k][i - 1])) return fail(c, -1, "mark %d: bin edges must increase", k);
  for (int k = 0; k < model->n_unit; ++k) {
    const mpp_unit_term &t = model->unit[k];
    if (t.kind != MPP_U_CONTRAST && t.kind != MPP_U_GRADIENT) continue;
    // the rasteriser works on a 96 x 128 pixel window: the largest rectangle (size = vmax, ratio -> 0) must fit with its margins
    if (!(maps->vmax[0] <= 36.0)) return fail(c, -1, "unit term %d: the classic image energies need size marks <= 36 px", k);
    if (t.kind == MPP_U_CONTRAST) {
      const int measure = (int)t.p[0], dil = (int)t.p[1], gap = (int)t.p[2], ero = (int)t.p[3];
      if (measure < 0 || measure > 5 || dil < 1 || dil > 4 || gap < 0 || gap > 2 || ero < 0 || ero > 2)
        return fail(c, -1, "unit term %d: contrast energy wants measure 0..5, dilation 1..4, gap 0..2, erode 0..2", k);
    }
  }
  c->hp.model = *model;
  c->hp.maps = *maps;
  c->have_model = true;
  c->remap_dirty = true;
  refresh_grid(c);
  return 0;
}

extern "C" int mpp_set_kernels(mpp_ctx *c, const mpp_kernels *k, const double *intensity) {
  if (!c || !k) return -1;
  double acc = 0.0;
  for (int i = 0; i < MPP_NKERNEL; ++i) {
    if (k->p_kernel[i] < 0) return fail(c, -1, "negative kernel probability");
    acc += k->p_kernel[i]; c->hp.p_cum[i] = acc;
  }
  if (fabs(acc - 1.0) > 1e-8) return fail(c, -1, "kernel probabilities do not sum to 1");   // make_kernels.py:164-172
  if (k->max_delta < 0 || k->max_delta > 15) return fail(c, -1, "max_delta must be in 0..15");
  // 8 kernels unless split / merge carry probability (the cumulative table is searched up to the last active one)
  c->hp.n_kernels = (k->p_kernel[MPP_K_SPLIT] > 0.0 || k->p_kernel[MPP_K_MERGE] > 0.0) ? MPP_NKERNEL : MPP_K_SPLIT;
  if (c->hp.n_kernels == MPP_NKERNEL && !(k->split_radius > 0.0 && k->split_sigma > 0.0))
    return fail(c, -1, "split/merge kernels need split_radius > 0 and split_sigma > 0");
  if (!c->have_kernels || c->hp.kern.max_delta != k->max_delta) c->box_dirty = c->win_dirty = true;
  c->hp.kern = *k;
  c->have_kernels = true;
  c->params_dirty = true;
  if (intensity) {
    c->intensity.assign(intensity, intensity + (c->n_tiles > 0 ? c->n_tiles : 1));
    c->tiles_dirty = true;
  }
  return 0;
}

extern "C" int mpp_set_maps(mpp_ctx *c, int n_tiles, int H, int W, const float *det, const float *m0, const float *m1,
                            const float *m2, int on_device) {
  if (!c) return -1;
  if (n_tiles <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return fail(c, -1, "bad tile geometry");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_tiles(c);
  c->n_maps = n_tiles; c->n_tiles = n_tiles * c->replicas; c->H = H; c->W = W;
  c->key_seed.clear(); c->key_chain.clear();
  c->ladder = false;                               // (its rungs went with the tiles' arrays)
  const size_t hw = (size_t)H * W, M = (size_t)n_tiles, T = (size_t)c->n_tiles;
  const float *src[4] = {det, m0, m1, m2};
  float **dst[4] = {&c->det, &c->m[0], &c->m[1], &c->m[2]};
  c->maps_borrowed = on_device != 0;
  for (int k = 0; k < 4; ++k) {
    size_t cnt = M * hw * (k == 0 ? 1 : MPP_NCLASS);
    if (on_device) {
      if (!src[k]) return fail(c, -1, "borrowed device maps must all be given");
      *dst[k] = const_cast<float *>(src[k]);
    } else {
      HIPCHK(c, hipMalloc((void **)dst[k], cnt * sizeof(float)));
      if (src[k]) HIPCHK(c, hipMemcpyAsync(*dst[k], src[k], cnt * sizeof(float), hipMemcpyHostToDevice, c->stream));
      else HIPCHK(c, hipMemsetAsync(*dst[k], 0, cnt * sizeof(float), c->stream));
    }
  }
  // (the cumulative tables of the birth kernels -- 16 B per pixel -- are made by the first chain launch: a context that only
  //  scores or merges, e.g. one whole 4096 x 4096 image, never needs them)
  c->cdf_ready = false;
  c->box_dirty = c->win_dirty = true;
  HIPCHK(c, c->px.alloc(T * c->cap)); HIPCHK(c, c->py.alloc(T * c->cap));
  HIPCHK(c, c->ps.alloc(T * c->cap)); HIPCHK(c, c->pr.alloc(T * c->cap)); HIPCHK(c, c->pa.alloc(T * c->cap));
  HIPCHK(c, c->n.alloc(T)); HIPCHK(c, c->errd.alloc(T)); HIPCHK(c, c->T.alloc(T * 3));
  HIPCHK(c, c->step.alloc(T)); HIPCHK(c, c->d_tiles.alloc(T)); HIPCHK(c, c->until.alloc(T));
  HIPCHK(c, hipMemsetAsync(c->n, 0, T * sizeof(int32_t), c->stream));
  HIPCHK(c, hipMemsetAsync(c->errd, 0, T * sizeof(int32_t), c->stream));
  HIPCHK(c, hipMemsetAsync(c->step, 0, T * sizeof(int64_t), c->stream));
  std::vector<double> sched(T * 3);
  for (size_t t = 0; t < T; ++t) { sched[3 * t] = c->sched[0]; sched[3 * t + 1] = c->sched[1]; sched[3 * t + 2] = c->sched[2]; }
  HIPCHK(c, hipMemcpyAsync(c->T, sched.data(), sched.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if ((int)c->intensity.size() != c->n_tiles) c->intensity.assign(c->n_tiles, 1.0);
  c->hbm_tile.assign(c->n_tiles, 0);
  c->lds_cap = c->lds_cell = 0;
  c->have_maps = true;
  c->tiles_dirty = true;
  refresh_grid(c);
  return 0;
}

extern "C" int mpp_set_image(mpp_ctx *c, int n_tiles, int C, const float *img, int on_device) {
  if (!c) return -1;
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  if (n_tiles != c->n_maps) return fail(c, -1, "mpp_set_image: %d tiles given, the ctx holds %d", n_tiles, c->n_maps);
  if (!img || (C != 1 && C != 2 && C != 3 && C != 6)) return fail(c, -1, "mpp_set_image: C must be 1, 2, 3 or 6");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->img && !c->img_borrowed) (void)hipFree(c->img);
  c->img = nullptr;
  const size_t cnt = (size_t)c->n_maps * c->H * c->W * C;
  if (on_device) c->img = const_cast<float *>(img);
  else {
    HIPCHK(c, hipMalloc((void **)&c->img, cnt * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->img, img, cnt * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  c->img_borrowed = on_device != 0;
  c->img_c = C;
  c->tiles_dirty = true;
  return 0;
}

int push_state(mpp_ctx *c) {
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  if (!c->have_model) return fail(c, -1, "mpp_set_model has not been called");
  {
    const ModelClass mc = model_class(c->hp);
    const bool grad = mc.gradient;
    if (mc.classic) {
      if (!c->img) return fail(c, -1, "the model has a classic image energy: mpp_set_image has not been called");
      if (grad ? (c->img_c != 2 && c->img_c != 6) : (c->img_c != 1 && c->img_c != 3))
        return fail(c, -1, "the image has %d channels: the %s energy wants %s", c->img_c, grad ? "gradient" : "contrast",
                    grad ? "2 or 6 (np.gradient)" : "1 or 3");
    }
  }
  HIPCHK(c, hipSetDevice(c->device));
  const bool win = c->window_rows && c->have_kernels && c->cdf_ready;
  if (win && !c->rowwin.p) {
    HIPCHK(c, c->rowwin.alloc(rowwin_count((size_t)c->n_maps, c->H, c->W)));
    c->win_dirty = true; c->tiles_dirty = true;
  }
  if (c->tiles_dirty) {
    const size_t hw = (size_t)c->H * c->W;
    c->h_tiles.resize(c->n_tiles);
    for (int t = 0; t < c->n_tiles; ++t) {
      TileRef &r = c->h_tiles[t];
      const size_t m = (size_t)(t % c->n_maps);                    // replica chains share their tile's maps
      r.det = (const MPP_GLOBAL float *)(c->det + m * hw);
      for (int k = 0; k < 3; ++k) r.m[k] = (const MPP_GLOBAL float *)(c->m[k] + m * hw * MPP_NCLASS);
      r.rowpart = c->cdf_ready ? (const MPP_GLOBAL double *)(c->rowpart + m * hw) : nullptr;
      r.rowbase = c->cdf_ready ? (const MPP_GLOBAL double *)(c->rowbase + m * (c->H + 1)) : nullptr;
      r.boxsum = c->cdf_ready ? (const MPP_GLOBAL double *)(c->boxsum + m * hw) : nullptr;
      r.rowwin = win ? (const MPP_GLOBAL double *)(c->rowwin + m * hw) : nullptr;
      for (int k = 0; k < 3; ++k)
        r.rm[k] = c->remap[k] ? (const MPP_GLOBAL double *)(c->remap[k] + m * hw * MPP_NCLASS) : nullptr;
      r.img = c->img ? (const MPP_GLOBAL float *)(c->img + m * hw * (size_t)c->img_c) : nullptr;
      r.img_c = c->img_c; r._pad_img = 0;
      r.px = c->px + (size_t)t * c->cap; r.py = c->py + (size_t)t * c->cap;
      r.ps = c->ps + (size_t)t * c->cap; r.pr = c->pr + (size_t)t * c->cap; r.pa = c->pa + (size_t)t * c->cap;
      r.n = c->n + t; r.T = c->T + 3 * (size_t)t; r.step = c->step + t; r.err = c->errd + t;
      r.intensity = c->intensity[t];
      const bool own = (int)c->key_seed.size() == c->n_tiles;
      r.key_on = own ? 1u : 0u; r.key_seed = own ? c->key_seed[t] : 0ull; r.key_chain = own ? c->key_chain[t] : 0u;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_tiles, c->h_tiles.data(), sizeof(TileRef) * c->n_tiles, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tiles_dirty = false;
  }
  if (c->box_dirty && c->have_kernels && c->cdf_ready) {
    mpp_launch_boxsum(c->stream, c->n_maps, c->rowpart, c->H, c->W, c->hp.kern.max_delta, c->boxsum);
    HIPCHK(c, hipGetLastError());
    c->box_dirty = false;
  }
  if (c->win_dirty && win) {
    mpp_launch_rowwin(c->stream, c->n_maps, c->rowpart, c->H, c->W, c->hp.kern.max_delta, c->rowwin);
    HIPCHK(c, hipGetLastError());
    c->win_dirty = false;
  }
  if (c->params_dirty) {
    c->hp.cap = c->cap; c->hp.cell_cap = c->cell_cap; c->hp.n_tiles = c->n_tiles;
    HIPCHK(c, hipMemcpyAsync(c->dp, &c->hp, sizeof(DevParams), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->params_dirty = false;
  }
  return 0;
}
int check_tile(mpp_ctx *c, int tile) {
  if (!c) return -1;
  if (!c->have_maps) return fail(c, -1, "mpp_set_maps has not been called");
  if (tile < 0 || tile >= c->n_tiles) return fail(c, -1, "tile %d out of range", tile);
  return 0;
}

extern "C" int mpp_set_chain_keys(mpp_ctx *c, int n, const uint64_t *seeds, const uint32_t *chains) {
  if (!c) return -1;
  if (!seeds || !chains) {                     // back to the launch's seed and chain0 + tile
    c->key_seed.clear(); c->key_chain.clear(); c->tiles_dirty = true;
    return 0;
  }
  if (!c->have_maps || n != c->n_tiles) return fail(c, -1, "mpp_set_chain_keys: one key per chain of the context (%d)", c->n_tiles);
  c->key_seed.assign(seeds, seeds + n); c->key_chain.assign(chains, chains + n);
  c->tiles_dirty = true;
  return 0;
}

extern "C" int mpp_set_points(mpp_ctx *c, int tile, int n, const int32_t *xy, const double *marks) {
  int rc = check_tile(c, tile);
  if (rc) return rc;
  if (n < 0 || n > c->cap) return fail(c, -4, "%d points exceed point_capacity %d", n, c->cap);
  std::vector<int32_t> x(n), y(n);
  std::vector<double> s(n), r(n), a(n);
  for (int i = 0; i < n; ++i) {
    x[i] = xy[2 * i]; y[i] = xy[2 * i + 1];
    if (x[i] < 0 || x[i] >= c->H || y[i] < 0 || y[i] >= c->W)
      return fail(c, -5, "point %d (%d,%d) is outside the %dx%d tile", i, x[i], y[i], c->H, c->W);  // point_set.py:99
    s[i] = marks[3 * i]; r[i] = marks[3 * i + 1]; a[i] = marks[3 * i + 2];
  }
  HIPCHK(c, hipSetDevice(c->device));
  size_t o = (size_t)tile * c->cap;
  HIPCHK(c, hipMemcpyAsync(c->px + o, x.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->py + o, y.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->ps + o, s.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pr + o, r.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->pa + o, a.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  int32_t nn = n, zero = 0;
  HIPCHK(c, hipMemcpyAsync(c->n + tile, &nn, sizeof nn, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->errd + tile, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int mpp_count(mpp_ctx *c, int tile, int32_t *n) {
  int rc = check_tile(c, tile);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(n, c->n + tile, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int mpp_get_points(mpp_ctx *c, int tile, int cap, int32_t *n_out, int32_t *xy, double *marks) {
  int32_t n = 0;
  int rc = mpp_count(c, tile, &n);
  if (rc) return rc;
  if (n_out) *n_out = n;
  int m = n < cap ? n : cap;
  if (m <= 0 || !xy || !marks) return 0;
  std::vector<int32_t> x(m), y(m);
  std::vector<double> s(m), r(m), a(m);
  size_t o = (size_t)tile * c->cap;
  HIPCHK(c, hipMemcpyAsync(x.data(), c->px + o, m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(y.data(), c->py + o, m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(s.data(), c->ps + o, m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(r.data(), c->pr + o, m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(a.data(), c->pa + o, m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < m; ++i) {
    xy[2 * i] = x[i]; xy[2 * i + 1] = y[i];
    marks[3 * i] = s[i]; marks[3 * i + 1] = r[i]; marks[3 * i + 2] = a[i];
  }
  return 0;
}

// every tile's configuration with five strided copies instead of six small ones per tile (256 tiles: 32 ms -> <1 ms)
extern "C" int mpp_get_points_all(mpp_ctx *c, int cap, int32_t *n_out, int32_t *xy, double *marks) {
  if (!c || c->n_tiles <= 0 || !n_out || cap < 0) return fail(c, -1, "bad get_points_all arguments");
  const int T = c->n_tiles;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(n_out, c->n, sizeof(int32_t) * T, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!xy || !marks || cap == 0) return 0;
  int m = 0;
  for (int t = 0; t < T; ++t) m = n_out[t] > m ? n_out[t] : m;
  m = m < cap ? m : cap;
  m = m < c->cap ? m : c->cap;
  if (m <= 0) return 0;
  std::vector<int32_t> x((size_t)T * m), y((size_t)T * m);
  std::vector<double> s((size_t)T * m), r((size_t)T * m), a((size_t)T * m);
  const size_t wi = (size_t)m * sizeof(int32_t), wd = (size_t)m * sizeof(double);
  const size_t pi = (size_t)c->cap * sizeof(int32_t), pd = (size_t)c->cap * sizeof(double);
  HIPCHK(c, hipMemcpy2DAsync(x.data(), wi, c->px, pi, wi, T, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(y.data(), wi, c->py, pi, wi, T, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(s.data(), wd, c->ps, pd, wd, T, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(r.data(), wd, c->pr, pd, wd, T, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(a.data(), wd, c->pa, pd, wd, T, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int t = 0; t < T; ++t) {
    const int k = n_out[t] < m ? n_out[t] : m;
    for (int i = 0; i < k; ++i) {
      const size_t src = (size_t)t * m + i, dst = (size_t)t * cap + i;
      xy[2 * dst] = x[src]; xy[2 * dst + 1] = y[src];
      marks[3 * dst] = s[src]; marks[3 * dst + 1] = r[src]; marks[3 * dst + 2] = a[src];
    }
  }
  return 0;
}

extern "C" int mpp_set_schedule(mpp_ctx *c, double T0, double alpha, double T_target) {
  if (!c) return -1;
  if (!(T0 >= T_target)) return fail(c, -1, "t0 must be >= t_target");          // rjmcmc.py:71
  c->sched[0] = T0; c->sched[1] = alpha; c->sched[2] = T_target;
  c->ladder = false;                               // every chain on the same schedule again: mpp_set_ladder sets a new one
  if (c->have_maps) {
    std::vector<double> sched((size_t)c->n_tiles * 3);
    for (int t = 0; t < c->n_tiles; ++t) { sched[3 * t] = T0; sched[3 * t + 1] = alpha; sched[3 * t + 2] = T_target; }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(c->T, sched.data(), sched.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->step, 0, c->n_tiles * sizeof(int64_t), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return 0;
}
