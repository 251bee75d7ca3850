// mpp_api_nets.hip -- the C ABI around the U-Nets, thin wrappers that check their arguments: inference (mpp_maps.hip,
// mpp_conv.hip; one entry point per score-map epilogue, its window form mpp_*_win), detection (mpp_detect.hip), training
// (mpp_train.hip, mpp_resample.hip), rescale (mpp_rescale.hip), and the result pictures (mpp_figures.hip).
#include "mpp_ctx.hpp"

extern "C" int mpp_affine_relu(mpp_ctx *c, void *x, int planes, int C, int64_t hw, int elem_bytes, const float *scale,
                               const float *shift) {
  if (!c || !x || !scale || !shift || planes <= 0 || C <= 0 || hw <= 0 || planes % C) return fail(c, -1, "bad affine_relu arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (mpp_launch_affine_relu(c->stream, x, planes, C, (size_t)hw, elem_bytes, scale, shift))
    return fail(c, -1, "affine_relu: element type must be float32 or bfloat16");
  HIPCHK(c, hipGetLastError());
  return 0;
}
extern "C" int mpp_nhwc_glue(mpp_ctx *c, const void *x0, const void *x1, void *y, int H, int W, int C0, int C1, int pad, int pool,
                             int in_bytes, int out_bytes, const float *scale, const float *shift) {
  if (!c || !x0 || !y || H <= 0 || W <= 0 || C0 <= 0 || C1 < 0 || (C1 > 0 && !x1) || (pad != 0 && pad != 1) || (pad && (H < 2 || W < 2)) ||
      (scale == nullptr) != (shift == nullptr))
    return fail(c, -1, "bad nhwc_glue arguments");
  if (y == x0 && (pad || pool || C1)) return fail(c, -1, "nhwc_glue: in place only without pad / pool / cat");
  HIPCHK(c, hipSetDevice(c->device));
  if (mpp_launch_nhwc_glue(c->stream, x0, C1 > 0 ? x1 : x0, y, H, W, C0, C1, pad, pool ? 1 : 0, in_bytes, out_bytes, scale, shift))
    return fail(c, -1, "nhwc_glue: element types must be float32 or bfloat16");
  HIPCHK(c, hipGetLastError());
  return 0;
}
extern "C" int mpp_conv3x3_c32(mpp_ctx *c, const float *x0, const float *x1, int H, int W, const float *wp, const float *in_scale,
                               const float *in_shift, const float *out_scale, const float *out_shift, int relu, float *y) {
  if (!c || !x0 || !wp || !y || H < 2 || W < 2 || (!in_scale) != (!in_shift) || (!out_scale) != (!out_shift))
    return fail(c, -1, "bad conv3x3_c32 arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (mpp_launch_conv3x3_c32(c->stream, x0, x1, H, W, wp, in_scale, in_shift, out_scale, out_shift, relu, y))
    return fail(c, -2, "conv3x3_c32 launch failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}

extern "C" int mpp_conv3x3_stem(mpp_ctx *c, const float *x, int H, int W, const float *wp, const float *scale, const float *shift,
                                float *y) {
  if (!c || !x || !wp || !scale || !shift || !y || H < 2 || W < 2) return fail(c, -1, "bad conv3x3_stem arguments");
  HIPCHK(c, hipSetDevice(c->device));
  if (mpp_launch_conv3x3_stem(c->stream, x, H, W, wp, scale, shift, y))
    return fail(c, -2, "conv3x3_stem launch failed (y must be 16-byte aligned): %s", hipGetErrorString(hipGetLastError()));
  return 0;
}
// ---- the CNN-only baseline's detection step (mpp_detect.hip) ------------------------------------------------------------
extern "C" int mpp_detect_centers(mpp_ctx *c, int H, int W, int ld, const float *det, double threshold, int strict,
                                  double nms_distance, int cap, int32_t *xy, float *scores, int64_t *n_candidates,
                                  int64_t *n_kept) {
  if (!c) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  return mpp_detect_run(c->stream, &c->detect, H, W, ld, det, threshold, strict, nms_distance, cap, xy, scores, n_candidates,
                        n_kept, &c->err);
}
extern "C" int mpp_mark_classes(mpp_ctx *c, int H, int W, int ld, const float *m0, const float *m1, const float *m2, int n,
                                const int32_t *xy, int32_t *classes) {
  if (!c || H < 0 || W < 0 || ld < W || n < 0 || (n > 0 && (!m0 || !m1 || !m2 || !xy || !classes)))
    return fail(c, -1, "bad mark_classes arguments");
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  mpp_launch_mark_classes(c->stream, H, W, ld, m0, m1, m2, n, xy, classes);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// ---- training the U-Nets (mpp_train.hip) ----------------------------------------------------------------------------
// what mpp_train_batch and mpp_train_aug_params ask of a batch's shape and of the augmentation flags (`who`: the caller's name)
static bool bad_batch_shape(int B, int P) { return B <= 0 || B > 65535 || P < 8 || P > MPP_TRAIN_MAX_P || (P & 1); }
static int bad_flags(mpp_ctx *c, const char *who, int flags, int P, const char *why) {
  if (flags & ~(MPP_AUG_GEOMETRIC | MPP_AUG_MEDIUM | MPP_AUG_STRONG | MPP_AUG_PERTURB | MPP_AUG_HISTMATCH | MPP_AUG_SPATIAL))
    return fail(c, -1, "%s: bad flags", who);
  if ((flags & MPP_AUG_SPATIAL) && (P % 8 || P < 32 || P > 512))
    return fail(c, -1, "%s: MPP_AUG_SPATIAL needs P %% 8 == 0 and 32 <= P <= 512%s, not P=%d", who, why, P);
  return 0;
}
extern "C" int mpp_train_batch(mpp_ctx *c, const mpp_train_data *data, const mpp_train_labels *labels, int B, int P,
                               const int32_t *desc, int flags, uint32_t seed, uint32_t epoch, uint32_t batch,
                               const mpp_train_out *out) {
  if (!c || !data || !labels || !out || !desc || !out->patch || !out->sums || !out->status)
    return fail(c, -1, "train_batch: missing arguments");
  if (bad_batch_shape(B, P)) return fail(c, -1, "train_batch: bad shape B=%d P=%d", B, P);
  if (data->n_images <= 0 || !data->images || !data->img_off || !data->img_hw || !data->obj_start || !data->centers ||
      !data->params)
    return fail(c, -1, "train_batch: no resident dataset");
  if (labels->kind == 0) {
    if (!(labels->sigma_dil > 0.0) || !(labels->max_distance >= 0.0)) return fail(c, -1, "train_batch: bad PosNet options");
  } else if (labels->kind == 1) {
    if (labels->n_classes < 1 || labels->n_classes > MPP_NCLASS) return fail(c, -1, "train_batch: n_classes must be in 1..32");
  } else {
    return fail(c, -1, "train_batch: kind must be 0 (PosNet) or 1 (ShapeNet)");
  }
  if (bad_flags(c, "train_batch", flags, P, " (CLAHE's 8 x 8 tiles)")) return -1;
  if ((flags & MPP_AUG_HISTMATCH) && (!c->train.hist || c->train.hist_images != data->n_images))
    return fail(c, -1, "train_batch: MPP_AUG_HISTMATCH needs the histograms of the data's %d images (mpp_train_set_histograms)",
                data->n_images);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_train_batch(c->stream, &c->train, *data, *labels, B, P, desc, flags, seed, epoch, batch, *out));
  return 0;
}
extern "C" int mpp_train_aug_params(mpp_ctx *c, int flags, uint32_t seed, uint32_t epoch, uint32_t batch, int B, int P,
                                    int n_images, mpp_aug_record *out) {
  if (!c || !out) return fail(c, -1, "train_aug_params: missing arguments");
  if (bad_batch_shape(B, P) || n_images <= 0)
    return fail(c, -1, "train_aug_params: bad shape B=%d P=%d n_images=%d", B, P, n_images);
  if (bad_flags(c, "train_aug_params", flags, P, "")) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_aug_params(c->stream, flags, seed, epoch, batch, B, P, n_images, out));
  return 0;
}
// ---- dataset translation: the anti-aliased rescale (mpp_rescale.hip) --------------------------------------------------------
extern "C" int mpp_rescale(mpp_ctx *c, const uint8_t *src, int H, int W, int64_t src_pitch, const int32_t *row_idx,
                           const double *row_w, int oh, int row_taps, const int32_t *col_idx, const double *col_w, int ow,
                           int col_taps, uint8_t *out, double *out_f64, int64_t workspace_limit) {
  if (!c) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  return mpp_rescale_run(c->stream, &c->rescale, src, H, W, src_pitch, row_idx, row_w, oh, row_taps, col_idx, col_w, ow, col_taps,
                         out, out_f64, workspace_limit, &c->err);
}
// ---- the result pictures (mpp_figures.hip): the small tables are the caller's host arrays, uploaded here; the call returns
// when the picture is complete, so they are free again ----------------------------------------------------------------------
extern "C" int mpp_draw_outlines(mpp_ctx *c, int H, int W, const float *rgb, const float *scalar, double vmin, double vmax,
                                 const float *lut, int n, const int32_t *corners, const float *colors, uint8_t *out) {
  if (!c || !out || H <= 0 || W <= 0 || H > 65536 || W > 65536 || n < 0 || n > (1 << 24) || (n > 0 && (!corners || !colors)))
    return fail(c, -1, "bad draw_outlines arguments");
  if ((rgb != nullptr) == (scalar != nullptr)) return fail(c, -1, "draw_outlines: give the RGB picture or the scalar map, not both");
  if (scalar && (!lut || !(vmax > vmin) || !(vmax - vmin < INFINITY)))
    return fail(c, -1, "draw_outlines: a scalar base needs a 256 x 3 table and finite vmin < vmax");
  for (size_t i = 0; i < (size_t)n * 8; ++i)
    if (corners[i] < -MPP_FIG_COORD_MAX || corners[i] > MPP_FIG_COORD_MAX)
      return fail(c, -1, "draw_outlines: corner %d of rectangle %d lies beyond +-%d", (int)(i / 2 % 4), (int)(i / 8), MPP_FIG_COORD_MAX);
  HIPCHK(c, hipSetDevice(c->device));
  // workspace: colours [n][3] float32, table [256][3] float32, corners [n][8] int32, then the owner image (16-byte aligned)
  const size_t col_b = (size_t)n * 3 * sizeof(float), lut_b = scalar ? 256 * 3 * sizeof(float) : 0, cor_b = (size_t)n * 8 * sizeof(int32_t);
  const size_t own_off = (col_b + lut_b + cor_b + 15) & ~(size_t)15;
  HIPCHK(c, c->figures.reserve(c->stream, own_off + (n > 0 ? (size_t)H * W * sizeof(int32_t) : 0)));
  unsigned char *ws = c->figures;
  if (n > 0) {
    HIPCHK(c, hipMemcpyAsync(ws, colors, col_b, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(ws + col_b + lut_b, corners, cor_b, hipMemcpyHostToDevice, c->stream));
  }
  if (scalar) HIPCHK(c, hipMemcpyAsync(ws + col_b, lut, lut_b, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, mpp_launch_draw_outlines(c->stream, H, W, rgb, scalar, vmin, vmax, (const float *)(ws + col_b), n,
                                     (const int32_t *)(ws + col_b + lut_b), (const float *)ws, (int32_t *)(ws + own_off), out));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
// ---- histogram matching and error-density resampling (mpp_train.hip, mpp_resample.hip) ----------------------------------
static bool no_dataset(const mpp_train_data *data) {
  return !data || data->n_images <= 0 || !data->images || !data->img_off || !data->img_hw;
}
extern "C" int mpp_image_histograms(mpp_ctx *c, const mpp_train_data *data, uint32_t *hist) {
  if (!c || no_dataset(data) || !hist) return fail(c, -1, "image_histograms: missing arguments");
  if (data->n_images > 65535) return fail(c, -1, "image_histograms: at most 65535 images");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_image_histograms(c->stream, *data, hist));
  return 0;
}
extern "C" int mpp_train_set_histograms(mpp_ctx *c, const uint32_t *hist, int n_images) {
  if (!c || (hist && n_images <= 0)) return fail(c, -1, "train_set_histograms: bad arguments");
  c->train.hist = hist;
  c->train.hist_images = hist ? n_images : 0;
  return 0;
}
extern "C" int mpp_posnet_error_map(mpp_ctx *c, int H, int W, int ldh, int ldw, const float *out, int cx0, int cy0, int x0, int x1,
                                    int y0, int y1, const int32_t *centers, int n, double max_distance, uint8_t *dens,
                                    unsigned long long *sum, float *cell_out) {
  if (!c || !out || !dens || !sum || n < 0 || (n > 0 && !centers)) return fail(c, -1, "posnet_error_map: missing arguments");
  if (H <= 0 || W <= 0 || ldh <= 0 || ldw <= 0 || !(max_distance >= 0.0) || max_distance > 1024.0)
    return fail(c, -1, "posnet_error_map: bad extent or max_distance");
  if (x0 < 0 || y0 < 0 || x0 >= x1 || y0 >= y1 || x1 > H || y1 > W || (x0 & 7) || (y0 & 7) || ((x1 & 7) && x1 != H) ||
      ((y1 & 7) && y1 != W))
    return fail(c, -1, "posnet_error_map: the core (%d, %d, %d, %d) must lie in the %d x %d image on multiples of 8", x0, x1, y0,
                y1, H, W);
  if (cx0 < 0 || cy0 < 0 || cx0 > x0 || cy0 > y0 || x1 - cx0 > ldh || y1 - cy0 > ldw)
    return fail(c, -1, "posnet_error_map: the core lies outside the %d x %d output at (%d, %d)", ldh, ldw, cx0, cy0);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_error_map(c->stream, H, W, ldh, ldw, out, cx0, cy0, x0, x1, y0, y1, centers, n, max_distance, dens, sum,
                                 cell_out));
  return 0;
}
extern "C" int mpp_density_prefix(mpp_ctx *c, int n_images, const int32_t *img_hw, const int64_t *cell_off, const int64_t *row_off,
                                  int64_t total_rows, const uint8_t *dens, uint32_t *cellcum, unsigned long long *rowcum) {
  if (!c || !img_hw || !cell_off || !row_off || !dens || !cellcum || !rowcum) return fail(c, -1, "density_prefix: missing arguments");
  if (n_images <= 0 || total_rows < n_images || total_rows > 0x7fffffff)
    return fail(c, -1, "density_prefix: bad counts (%d images, %lld rows)", n_images, (long long)total_rows);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_density_prefix(c->stream, n_images, img_hw, cell_off, row_off, total_rows, dens, cellcum, rowcum));
  return 0;
}
extern "C" int mpp_density_anchors(mpp_ctx *c, int n_images, const int32_t *img_hw, const int64_t *cell_off, const int64_t *row_off,
                                   const uint32_t *cellcum, const unsigned long long *rowcum, int n, const int32_t *rows,
                                   uint32_t seed, uint32_t epoch, int32_t *anchors) {
  if (!c || !img_hw || !cell_off || !row_off || !cellcum || !rowcum || n < 0 || (n > 0 && (!rows || !anchors)) || n_images <= 0)
    return fail(c, -1, "density_anchors: bad arguments");
  if (n == 0) return 0;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_density_anchors(c->stream, n_images, img_hw, cell_off, row_off, cellcum, rowcum, n, rows, seed, epoch,
                                       anchors));
  return 0;
}
extern "C" int mpp_posnet_loss(mpp_ctx *c, int B, int P, const float *out, const float *vec, const float *mask, const float *dil,
                               const double *sums, int with_div, const float *w, const float *b, float *grad, double *res) {
  if (!c || !out || !vec || !mask || !sums || !res || (with_div && (!dil || !w || !b)))
    return fail(c, -1, "posnet_loss: missing arguments");
  if (B <= 0 || B > 65535 || P < 3 || P > MPP_TRAIN_MAX_P) return fail(c, -1, "posnet_loss: bad shape B=%d P=%d", B, P);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_posnet_loss(c->stream, &c->train, B, P, out, vec, mask, dil, sums, with_div ? 1 : 0, w, b, grad, res));
  return 0;
}
extern "C" int mpp_shapenet_loss(mpp_ctx *c, int B, int P, int n_classes, const float *l0, const float *l1, const float *l2,
                                 const uint8_t *cls, const uint8_t *cover, const double *sums, float *g0, float *g1, float *g2,
                                 double *res) {
  if (!c || !l0 || !l1 || !l2 || !cls || !cover || !sums || !res || (!g0 != !g1) || (!g1 != !g2))
    return fail(c, -1, "shapenet_loss: missing arguments");
  if (B <= 0 || B > 65535 || P < 1 || P > MPP_TRAIN_MAX_P || n_classes < 1 || n_classes > MPP_NCLASS)
    return fail(c, -1, "shapenet_loss: bad shape B=%d P=%d n_classes=%d", B, P, n_classes);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, mpp_launch_shapenet_loss(c->stream, &c->train, B, P, n_classes, l0, l1, l2, cls, cover, sums, g0, g1, g2, res));
  return 0;
}

// ---- the U-Net epilogues: the window (wx0, wy0, wh x ww) of an H x W crop into a full-image map, one entry point and one kernel
// per epilogue; the whole crop is the window (0, 0, H x W) with a dense destination (ld = W) ------------------------------------
static int bad_window(mpp_ctx *c, const char *what, int H, int W, int ldh, int ldw, int wx0, int wy0, int wh, int ww, int ld_dst) {
  if (H <= 0 || W <= 0 || ldh < H || ldw < W) return fail(c, -1, "%s: bad crop extent", what);
  if (wx0 < 0 || wy0 < 0 || wh <= 0 || ww <= 0 || wx0 > H - wh || wy0 > W - ww)
    return fail(c, -1, "%s: window (%d, %d, %d x %d) outside the %d x %d crop", what, wx0, wy0, wh, ww, H, W);
  if (ld_dst < ww) return fail(c, -1, "%s: destination pitch %d smaller than the window width %d", what, ld_dst, ww);
  return 0;
}
extern "C" int mpp_posnet_epilogue_win(mpp_ctx *c, int H, int W, int ldh, int ldw, const float *pos_out, double div_w, double div_b,
                                       int wx0, int wy0, int wh, int ww, float *det, int ld_det) {
  if (!c || !pos_out || !det) return fail(c, -1, "bad epilogue arguments");
  if (bad_window(c, "posnet_epilogue_win", H, W, ldh, ldw, wx0, wy0, wh, ww, ld_det)) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  mpp_launch_posnet_epilogue(c->stream, pos_out, H, W, ldh, ldw, (float)div_w, (float)div_b, wx0, wy0, wh, ww, det, ld_det);
  HIPCHK(c, hipGetLastError());
  return 0;
}
extern "C" int mpp_shapenet_epilogue_win(mpp_ctx *c, int H, int W, int ldh, int ldw, const float *logits, int wx0, int wy0, int wh, int ww,
                                         float *marks, int ld_marks) {
  if (!c || !logits || !marks) return fail(c, -1, "bad epilogue arguments");
  if (bad_window(c, "shapenet_epilogue_win", H, W, ldh, ldw, wx0, wy0, wh, ww, ld_marks)) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  if (mpp_launch_shapenet_epilogue(c->stream, logits, ldh, ldw, wx0, wy0, wh, ww, marks, ld_marks))
    return fail(c, -1, "shapenet_epilogue_win: marks must be 16-byte aligned");
  HIPCHK(c, hipGetLastError());
  return 0;
}
extern "C" int mpp_posnet_epilogue_nhwc_win(mpp_ctx *c, int H, int W, int ldh, int ldw, const void *pos_out, int elem_bytes, double div_w,
                                            double div_b, int wx0, int wy0, int wh, int ww, float *det, int ld_det) {
  if (!c || !pos_out || !det) return fail(c, -1, "bad epilogue arguments");
  if (bad_window(c, "posnet_epilogue_nhwc_win", H, W, ldh, ldw, wx0, wy0, wh, ww, ld_det)) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  if (mpp_launch_posnet_epilogue_nhwc(c->stream, pos_out, elem_bytes, H, W, ldw, (float)div_w, (float)div_b, wx0, wy0, wh, ww, det,
                                      ld_det))
    return fail(c, -1, "posnet_epilogue_nhwc_win: element type must be float32 or bfloat16");
  HIPCHK(c, hipGetLastError());
  return 0;
}
extern "C" int mpp_shapenet_epilogue_nhwc_win(mpp_ctx *c, int H, int W, int ldh, int ldw, const void *logits, int elem_bytes, int wx0,
                                              int wy0, int wh, int ww, float *marks, int ld_marks) {
  if (!c || !logits || !marks) return fail(c, -1, "bad epilogue arguments");
  if (bad_window(c, "shapenet_epilogue_nhwc_win", H, W, ldh, ldw, wx0, wy0, wh, ww, ld_marks)) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  const int e = mpp_launch_shapenet_epilogue_nhwc(c->stream, logits, elem_bytes, ldw, wx0, wy0, wh, ww, marks, ld_marks);
  if (e == -1) return fail(c, -1, "shapenet_epilogue_nhwc_win: element type must be float32 or bfloat16");
  if (e == -2) return fail(c, -1, "shapenet_epilogue_nhwc_win: logits and marks must be 16-byte aligned");
  HIPCHK(c, hipGetLastError());
  return 0;
}
extern "C" int mpp_shapenet_heads_win(mpp_ctx *c, int H, int W, int ldh, int ldw, const float *h, const float *w, const float *b, int wx0,
                                      int wy0, int wh, int ww, float *marks_size, float *marks_ratio, float *marks_angle, int ld_marks) {
  if (!c || !h || !w || !b || !marks_size || !marks_ratio || !marks_angle) return fail(c, -1, "bad shapenet_heads arguments");
  if (bad_window(c, "shapenet_heads_win", H, W, ldh, ldw, wx0, wy0, wh, ww, ld_marks)) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  const int rc = mpp_launch_shapenet_heads(c->stream, h, ldw, w, b, wx0, wy0, wh, ww, marks_size, marks_ratio, marks_angle, ld_marks);
  if (rc == -2 && (((uintptr_t)h | (uintptr_t)marks_size | (uintptr_t)marks_ratio | (uintptr_t)marks_angle) & 15))
    return fail(c, -1, "shapenet_heads_win: the activations and the mark maps must be 16-byte aligned");
  if (rc) return fail(c, -2, "shapenet_heads_win launch failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}
