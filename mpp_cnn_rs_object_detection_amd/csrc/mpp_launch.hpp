// mpp_launch.hpp -- the host launchers and LDS-size functions of the kernel files, declared once and included by the file that
// defines each and by the API files that call them: extern "C" symbols link whatever their prototype says, here a drift fails to compile.
#pragma once
#include <cstddef>

#include "mpp_device.hpp"
#include "mpp_prepass.hpp"

#define MPP_LDS_LIMIT (160 * 1024)                 // the LDS of a CU: what a chain's dynamic + static LDS has to fit
#define MPP_DEDUPE_LDS_MAX (MPP_LDS_LIMIT - 256)   // the most the dedupe walk of mpp_merge_score may ask for (k_dedupe_tiles)

extern "C" {
size_t mpp_chain_lds_bytes(int cap, int ncell, int cell_cap, int spec, int rowbase_n, int waves);
size_t mpp_chain_static_lds_bytes(int waves);
size_t mpp_chain_hbm_state_bytes(int cap, int ncell, int cell_cap);
size_t mpp_chain_hbm_lds_bytes(int spec, int rowbase_n);
hipError_t mpp_launch_chain_hbm(hipStream_t st, int waves, int grid, size_t lds, const DevParams *P, const TileRef *tiles,
                                int tile0, const long long *until, long long trace_base, unsigned long long seed,
                                unsigned int chain0, const mpp_proposal *tape, int trace_tile, mpp_step_out *out,
                                mpp_proposal *props, unsigned char *ws, size_t ws_stride);
hipError_t mpp_launch_chain(hipStream_t st, int spec, int lanes, int occ, int grid, size_t lds, const DevParams *P,
                            const TileRef *tiles, int tile0, const long long *until, long long trace_base,
                            unsigned long long seed, unsigned int chain0, const mpp_proposal *tape, int trace_tile,
                            mpp_step_out *out, mpp_proposal *props);
hipError_t mpp_launch_hot(hipStream_t st, int grid, size_t lds, const DevParams *P, const TileRef *tiles, int tile0,
                          const long long *until, const PreTab *pt);
size_t mpp_deep_lds_bytes(int cap, int ncell, int cell_cap, int rowbase_n, int waves, int nmax, int ext);
size_t mpp_deep_static_lds_bytes(int waves);
hipError_t mpp_launch_deep(hipStream_t st, int waves, int occ, int grid, size_t lds, const DevParams *P, const TileRef *tiles,
                           int tile0, const long long *until, long long trace_base, unsigned long long seed, unsigned int chain0,
                           int trace_tile, mpp_step_out *out, mpp_proposal *props, int nmax, int fixed_depth, int gain8,
                           unsigned long long *stats, int ext, const PreTab *pt);
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
void mpp_launch_cdf(hipStream_t st, int n_tiles, const float *det, int H, int W, double *rowpart, double *rowbase,
                    double *scratch_rowtot);
void mpp_launch_boxsum(hipStream_t st, int n_tiles, const double *rowpart, int H, int W, int md, double *boxsum);
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
