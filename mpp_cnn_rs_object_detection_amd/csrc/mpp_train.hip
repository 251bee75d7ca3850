// mpp_train.hip -- training the U-Nets: one launch builds a batch (crop, augmentation, labels), one launch per net computes
// the loss and its gradient.
//
//  * k_train_batch: one workgroup per (patch, band of MPP_TRAIN_BAND rows).  It compacts the objects of its image that fall
//    in the patch into LDS (a block-wide ballot scan keeps annotation order), moves them by the patch's D4 element, then
//    every thread labels its pixels against the LDS list: exact nearest centre for PosNet (ties to the lowest annotation
//    index), the even-odd crossing test of skimage.draw.polygon for ShapeNet (the rule csrc/mpp_classics.hpp restates).
//    It writes the band's label sums, so that the loss kernel knows both balancing betas before it writes a gradient.
//  * k_hist_lut (MPP_AUG_HISTMATCH only), in front of it: one workgroup per patch builds the patch's histogram in LDS and
//    the matching table of the patch's template image, lut [B][3][256] float32, which the band workgroups then apply.
//  * k_aug_spatial (MPP_AUG_SPATIAL only), between the two: one workgroup per patch whose draws pick at least one of the six
//    ops that need neighbours or the whole patch (shadow, fog, CLAHE, downscale, median / box blur); the others leave at
//    once.  It carries the image through the recipe up to the Gauss noise, stage by stage through a ping-pong pair of float32
//    patch buffers in a workspace of the ctx, a workgroup barrier between stages; the CLAHE tile histograms / tables, the
//    shadow vertices and the haze points live in LDS.  The band workgroups of k_train_batch then take the finished pixel of
//    such a patch from the workspace and add the noise.
//  * k_posnet_loss / k_shapenet_loss: one workgroup per (patch, band); each writes the loss and dL/dout of its pixels and
//    its partial sums, and the last workgroup to finish reduces the partials in a fixed order (the same inputs give the
//    same bits).
//
// Random draws: Philox4x32-10, key (seed, epoch), counter (batch, patch, stream, index); stream 0: the patch's draws,
// 1: class perturbation of an object (index: its row in the dataset's object table), 2: pixel noise (index: pixel).
// 3: the lists of the spatial ops (index 0..9: shadow vertex v of polygon v / 5, words 0, 1 = x, y; index 16 + k: haze point
// k, words 0, 1 = x, y).
// Stream 0's indices: 0 D4, 1..4 the photometric ops, 5 histogram matching, 6 and 7 the spatial ops:
//   6: word 0 shadow applies (u < 0.5), 1 two polygons (u < 0.5) else one, 2 fog applies (u < 0.5), 3 fog_coef = 0.3 + 0.7 u
//   7: word 0 CLAHE's clip = 1 + 3 u, 1 downscale applies (u < 0.5), 2 the blur OneOf fires (u < 0.2), 3 median (u < 0.5) else box
// (whether CLAHE applies is the colour OneOf's own draw, index 2 words 2 and 3, as before).
#include <cmath>
#include <cstdint>

#include "mpp_device.hpp"
#include "mpp_train.hpp"
#include "mpp_unet_math.hpp"

namespace {

constexpr int TB = 256;                    // threads of every workgroup here but k_aug_spatial's
constexpr int TS = 1024;                   // threads of a k_aug_spatial workgroup (one patch)
constexpr int MAXH = MPP_AUG_MAX_HAZE;
constexpr int BAND = MPP_TRAIN_BAND;
constexpr int MAXO = MPP_TRAIN_MAX_OBJ;
constexpr double PI = 3.14159265358979311600;   // np.pi

__device__ __forceinline__ double unif(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }   // (0, 1)

struct Rng {
  uint32_t k0, k1, batch, patch;
  __device__ void draw(uint32_t stream, uint32_t index, uint32_t o[4]) const {
    philox4x32_10(batch, patch, stream, index, k0, k1, o);
  }
};

// D4 element: rotation by k * 90 degrees as np.rot90 (pixel (r, c) -> (P-1-c, r)), then flip 0 none, 1 vertical (rows),
// 2 horizontal (columns), 3 both
__device__ __forceinline__ void d4_fwd(int k, int flip, int P, int &r, int &c) {
  for (int i = 0; i < k; ++i) {
    const int t = r;
    r = P - 1 - c;
    c = t;
  }
  if (flip & 1) r = P - 1 - r;
  if (flip & 2) c = P - 1 - c;
}
__device__ __forceinline__ void d4_inv(int k, int flip, int P, int &r, int &c) {
  if (flip & 1) r = P - 1 - r;
  if (flip & 2) c = P - 1 - c;
  for (int i = 0; i < k; ++i) {
    const int t = c;
    c = P - 1 - r;
    r = t;
  }
}
// the angle of the transformed rectangle: its rect_to_poly polygon is the D4 image of the original one; then % pi
__device__ __forceinline__ double d4_angle(int k, int flip, double a) {
  double t = a + (double)k * (PI / 2);
  if (flip == 1 || flip == 2) t = -t;
  else if (flip == 3) t = t + PI;
  double m = fmod(t, PI);
  if (m < 0) m += PI;
  if (m >= PI) m -= PI;
  return m;
}

// value -> class: the last lower bin edge the value reaches (mappings.py value_to_class)
__device__ __forceinline__ int value_class(const double *edges, int n, double v) {
  int c = -1;
  for (int i = 0; i < n; ++i) c += (edges[i] <= v) ? 1 : 0;
  return c < 0 ? 0 : c;
}

__device__ __forceinline__ float clip255(float x) { return fminf(fmaxf(x, 0.f), 255.f); }

struct PatchAug {
  int rot = 0, flip = 0;
  int chan_op = 0, chan_arg = 0;          // 1 shuffle (permutation chan_arg of 6), 2 dropout (channel chan_arg)
  int bc = 0; float alpha = 1.f, beta = 0.f;
  int color = 0; float shift[3] = {0.f, 0.f, 0.f};   // 1 RGB shift, 2 to gray
  int noise = 0; double sigma = 0.0;
  int hm = 0, tmpl = 0; double blend = 0.0;          // histogram matching to image tmpl
  // MPP_AUG_SPATIAL
  int shadow = 0, n_poly = 0;                        // RandomShadow with n_poly polygons
  int fog = 0; double fog_coef = 0.0;                // RandomFog
  int clahe = 0; double clip = 0.0;                  // CLAHE (the colour OneOf's first member)
  int down = 0;                                      // Downscale(0.9)
  int blur = 0;                                      // 1 MedianBlur(3), 2 Blur(3)
  __device__ bool spatial() const { return shadow | fog | clahe | down | blur; }
};

// the three draws of histogram matching (HistogramMatching(blend_ratio (0.1, 0.75), p 0.5), data/augmentation.py:26-29)
__device__ __forceinline__ void hist_draws(const Rng &g, int n_images, PatchAug &a) {
  uint32_t d[4];
  g.draw(0, 5, d);
  a.hm = unif(d[0]) < 0.5;
  a.tmpl = min(n_images - 1, (int)(unif(d[1]) * (double)n_images));
  a.blend = 0.1 + unif(d[2]) * 0.65;
}

// albumentations' defaults (RandomRotate90, Flip, ChannelShuffle, ChannelDropout((1, 1), fill 0), RandomBrightnessContrast
// (0.2, 0.2, brightness_by_max), RGBShift(20, 20, 20), ToGray, GaussNoise(var_limit (10, 50), mean 0, per channel)),
// composed as data/augmentation.py:22-72 lays them out; with MPP_AUG_SPATIAL also RandomShadow(), RandomFog(), CLAHE(),
// Downscale(0.9, 0.9, nearest), OneOf([MedianBlur(3), Blur(3)], p 0.2), as DESIGN.md section 8 defines them
__device__ PatchAug patch_draws(const Rng &g, int flags, int n_images) {
  PatchAug a;
  uint32_t d[4];
  if (flags & MPP_AUG_HISTMATCH) hist_draws(g, n_images, a);
  if (flags & MPP_AUG_GEOMETRIC) {
    g.draw(0, 0, d);
    a.rot = unif(d[0]) < 0.5 ? (int)(unif(d[1]) * 4.0) : 0;
    a.flip = unif(d[2]) < 0.5 ? 1 + (int)(unif(d[3]) * 3.0) : 0;
  }
  if (!(flags & (MPP_AUG_MEDIUM | MPP_AUG_STRONG))) return a;
  const bool strong = flags & MPP_AUG_STRONG;
  g.draw(0, 1, d);
  if (strong && unif(d[0]) < 0.5) {                       // OneOf([ChannelShuffle(), ChannelDropout()])
    a.chan_op = unif(d[1]) < 0.5 ? 1 : 2;
    a.chan_arg = (int)(unif(d[2]) * (a.chan_op == 1 ? 6.0 : 3.0));
  }
  if (strong && unif(d[3]) < 0.5) a.bc = 1;               // RandomBrightnessContrast()
  g.draw(0, 2, d);
  a.alpha = (float)(1.0 + (unif(d[0]) * 0.4 - 0.2));
  a.beta = (float)((unif(d[1]) * 0.4 - 0.2) * 255.0);
  if (unif(d[2]) < 0.5) {                                  // OneOf([CLAHE(), RGBShift()] (+ ToGray(p=0.1) when strong))
    const double w = unif(d[3]) * (strong ? 1.1 : 1.0);
    a.color = w < 0.5 ? 0 : (w < 1.0 ? 1 : 2);            // 0: CLAHE (applied with MPP_AUG_SPATIAL only)
    a.clahe = (flags & MPP_AUG_SPATIAL) && a.color == 0;
  }
  g.draw(0, 3, d);
  for (int ch = 0; ch < 3; ++ch) a.shift[ch] = (float)(unif(d[ch]) * 40.0 - 20.0);
  a.noise = unif(d[3]) < 0.5;                              // GaussNoise()
  g.draw(0, 4, d);
  a.sigma = sqrt(10.0 + unif(d[0]) * 40.0);
  if (!(flags & MPP_AUG_SPATIAL)) return a;
  g.draw(0, 6, d);
  if (strong) {
    a.shadow = unif(d[0]) < 0.5;                           // RandomShadow(): shadow_roi (0, 0.5, 1, 1), 1..2 polygons of 5
    a.n_poly = a.shadow ? 1 + (unif(d[1]) < 0.5 ? 1 : 0) : 0;
    a.fog = unif(d[2]) < 0.5;                              // RandomFog(): fog_coef U(0.3, 1), alpha_coef 0.08
    a.fog_coef = 0.3 + unif(d[3]) * 0.7;
  }
  g.draw(0, 7, d);
  a.clip = 1.0 + unif(d[0]) * 3.0;                         // CLAHE(): clip_limit U(1, 4), tile grid 8 x 8
  if (strong) a.down = unif(d[1]) < 0.5;                   // Downscale(0.9, 0.9)
  if (unif(d[2]) < 0.2) a.blur = unif(d[3]) < 0.5 ? 1 : 2; // OneOf([MedianBlur(3), Blur(3)], p 0.2)
  return a;
}

// randint(lo, hi), both ends included, from one word
__device__ __forceinline__ int rand_int(uint32_t w, int lo, int hi) {
  return min(hi, lo + (int)(unif(w) * (double)(hi - lo + 1)));
}
// shadow vertex v (0..9; polygon v / 5): x in [0, P], y in [P/2, P]
__device__ __forceinline__ void shadow_vertex(const Rng &g, int P, int v, int &x, int &y) {
  uint32_t d[4];
  g.draw(3, (uint32_t)v, d);
  x = rand_int(d[0], 0, P);
  y = rand_int(d[1], P / 2, P);
}
// The haze points of RandomFog as albumentations' loop lists them: rounds index = 1, 2, ... of (hw / 10) * index points in
// the window [midx, P - midx - hw] x [midy, P - midy - hw], which grows by 3 hw / 2 a side per round until it has passed the
// patch by hw on both axes.  Returns their number (the same for every k) and, for k below it, point k.  The count depends
// on (P, hw) alone; over every P <= 512 that is a multiple of 8 and every hw in 1 .. P / 3 its maximum is 51 (P = 512,
// hw = 170: rounds of 17 and 34), so MPP_AUG_MAX_HAZE = 64 cannot be reached; the loop stops there all the same.
__device__ __forceinline__ int fog_hw(int P, double coef) { return max(1, (int)((double)(P / 3) * coef)); }
__device__ int haze_point(const Rng &g, int P, double coef, int k, int &x, int &y) {
  const int hw = fog_hw(P, coef), per = hw / 10, dec = 3 * hw * P / (2 * P);
  int midx = P / 2 - 2 * hw, midy = P / 2 - hw, n = 0;
  for (int index = 1; (midx > -hw || midy > -hw) && n < MAXH; ++index) {
    const int m = min(per * index, MAXH - n);
    if (k >= n && k < n + m) {
      uint32_t d[4];
      g.draw(3, (uint32_t)(16 + k), d);
      x = rand_int(d[0], midx, P - midx - hw);
      y = rand_int(d[1], midy, P - midy - hw);
    }
    n += m;
    midx -= dec;
    midy -= dec;
  }
  return n;
}

// the ops between fog and CLAHE / downscale: channel shuffle | dropout, brightness / contrast, RGB shift | to gray
__device__ __forceinline__ void photometric_color(const PatchAug &a, float x[3]) {
  if (a.chan_op == 1) {
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const float y0 = x[perm[a.chan_arg][0]], y1 = x[perm[a.chan_arg][1]], y2 = x[perm[a.chan_arg][2]];
    x[0] = y0; x[1] = y1; x[2] = y2;
  } else if (a.chan_op == 2) {
    x[a.chan_arg] = 0.f;
  }
  if (a.bc)
    for (int ch = 0; ch < 3; ++ch) x[ch] = clip255(a.alpha * x[ch] + a.beta);
  if (a.color == 1) {
    for (int ch = 0; ch < 3; ++ch) x[ch] = clip255(x[ch] + a.shift[ch]);
  } else if (a.color == 2) {
    const float y = clip255(0.299f * x[0] + 0.587f * x[1] + 0.114f * x[2]);
    x[0] = x[1] = x[2] = y;
  }
}
__device__ __forceinline__ void photometric_noise(const PatchAug &a, const Rng &g, int pix, float x[3]) {
  if (a.noise) {
    uint32_t d[4];
    g.draw(2, (uint32_t)pix, d);
    const double r0 = sqrt(-2.0 * log(unif(d[0]))), r1 = sqrt(-2.0 * log(unif(d[2])));
    const double t0 = 2.0 * PI * unif(d[1]), t1 = 2.0 * PI * unif(d[3]);
    const double z[3] = {r0 * cos(t0), r0 * sin(t0), r1 * cos(t1)};
    for (int ch = 0; ch < 3; ++ch) x[ch] = clip255((float)((double)x[ch] + a.sigma * z[ch]));
  }
}
__device__ __forceinline__ void photometric(const PatchAug &a, const Rng &g, int pix, float x[3]) {
  photometric_color(a, x);
  photometric_noise(a, g, pix, x);
}

// where a patch is read from: its image and the top-left corner of the crop
struct PatchSrc {
  bool valid;
  int tl_r, tl_c, H, W;
  const uint8_t *im;
};
__device__ __forceinline__ PatchSrc patch_src(const mpp_train_data &data, const int32_t *desc, int b, int P) {
  PatchSrc s;
  const int img = desc[3 * b];
  s.valid = img >= 0 && img < data.n_images;
  s.tl_r = desc[3 * b + 1] - P / 2;
  s.tl_c = desc[3 * b + 2] - P / 2;
  s.H = s.valid ? data.img_hw[2 * img] : 0;
  s.W = s.valid ? data.img_hw[2 * img + 1] : 0;
  s.im = s.valid ? data.images + data.img_off[img] : nullptr;
  return s;
}
// pixel (i, j) of the patch after D4 and histogram matching: a read at tl + (source pixel), zeros outside the image
__device__ __forceinline__ void source_pixel(const PatchSrc &s, const PatchAug &aug, int flags, int P, int i, int j,
                                             const float (*hm_lut)[256], float x[3]) {
  int si = i, sj = j;
  if (flags & MPP_AUG_GEOMETRIC) d4_inv(aug.rot, aug.flip, P, si, sj);
  const int gr = s.tl_r + si, gc = s.tl_c + sj;
  x[0] = x[1] = x[2] = 0.f;
  if (s.valid && gr >= 0 && gr < s.H && gc >= 0 && gc < s.W) {
    const uint8_t *p = s.im + ((size_t)gr * s.W + gc) * 3;
    x[0] = (float)p[0]; x[1] = (float)p[1]; x[2] = (float)p[2];
  }
  if (aug.hm)                                               // one rounding: the blend is formed in float64
    for (int ch = 0; ch < 3; ++ch)
      x[ch] = clip255((float)(aug.blend * (double)hm_lut[ch][(int)x[ch]] + (1.0 - aug.blend) * (double)x[ch]));
}

// exclusive block-wide prefix of one flag per thread (TB threads); returns the total
__device__ __forceinline__ int block_scan(bool flag, int *wave_cnt, int &prefix) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  const int below = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wave_cnt[wave] = __popcll(bal);
  __syncthreads();
  int off = 0, total = 0;
  for (int w = 0; w < TB / 64; ++w) {
    off += (w < wave) ? wave_cnt[w] : 0;
    total += wave_cnt[w];
  }
  __syncthreads();
  prefix = off + below;
  return total;
}

__device__ __forceinline__ double block_sum(double v, double *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = TB / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// inclusive prefix of one uint32 per thread over the TB (= 256) threads, through buf
__device__ __forceinline__ uint32_t scan256(uint32_t v, uint32_t *buf) {
  buf[threadIdx.x] = v;
  __syncthreads();
  for (int s = 1; s < TB; s <<= 1) {
    const uint32_t add = (int)threadIdx.x >= s ? buf[threadIdx.x - s] : 0u;
    __syncthreads();
    buf[threadIdx.x] += add;
    __syncthreads();
  }
  const uint32_t r = buf[threadIdx.x];
  __syncthreads();
  return r;
}

// The matching table of every patch whose draw says "apply": thread v owns the 8-bit value v.  The patch's histogram is
// that of its in-image pixels plus its zero padding (D4 does not change a histogram); the template's comes from hist.
// lut[v] = np.interp(src_q[v], tmpl_q, tmpl_values) in float64, over the template's present values only.
__global__ __launch_bounds__(TB) void k_hist_lut(mpp_train_data data, int P, const int32_t *desc, const uint32_t *hist,
                                                 uint32_t seed, uint32_t epoch, uint32_t batch, float *lut) {
  __shared__ uint32_t cnt[3][256];
  __shared__ uint32_t buf[TB];
  __shared__ uint32_t t_cnt[256];
  __shared__ double t_q[256];
  const int b = blockIdx.x, v = threadIdx.x;
  const Rng g{seed, epoch, batch, (uint32_t)b};
  PatchAug aug;
  hist_draws(g, data.n_images, aug);
  if (!aug.hm) return;
  const int img = desc[3 * b];
  const bool valid = img >= 0 && img < data.n_images;
  const int tl_r = desc[3 * b + 1] - P / 2, tl_c = desc[3 * b + 2] - P / 2;
  const int H = valid ? data.img_hw[2 * img] : 0, W = valid ? data.img_hw[2 * img + 1] : 0;
  const uint8_t *im = valid ? data.images + data.img_off[img] : nullptr;
  for (int ch = 0; ch < 3; ++ch) cnt[ch][v] = 0u;
  __syncthreads();
  // the rows and columns of the patch that lie in the image
  const int ra = max(0, -tl_r), rb = min(P, H - tl_r), ca = max(0, -tl_c), cb = min(P, W - tl_c);
  const int nr = max(0, rb - ra), nc = max(0, cb - ca);
  for (int idx = threadIdx.x; idx < nr * nc; idx += TB) {
    const int gr = tl_r + ra + idx / nc, gc = tl_c + ca + idx % nc;
    const uint8_t *p = im + ((size_t)gr * W + gc) * 3;
    atomicAdd(&cnt[0][p[0]], 1u);
    atomicAdd(&cnt[1][p[1]], 1u);
    atomicAdd(&cnt[2][p[2]], 1u);
  }
  __syncthreads();
  const uint32_t pad = (uint32_t)(P * P - nr * nc);
  const double s_size = (double)P * (double)P;
  const double t_size = (double)data.img_hw[2 * aug.tmpl] * (double)data.img_hw[2 * aug.tmpl + 1];
  for (int ch = 0; ch < 3; ++ch) {
    const uint32_t s_cum = scan256(cnt[ch][v] + (v == 0 ? pad : 0u), buf);
    const uint32_t tc = hist[((size_t)aug.tmpl * 3 + ch) * 256 + v];
    const uint32_t t_cum = scan256(tc, buf);
    t_cnt[v] = tc;
    t_q[v] = (double)t_cum / t_size;
    __syncthreads();
    const double x = (double)s_cum / s_size;
    // j: the last present value whose quantile is <= x; j2: the next present value
    int first = -1, last = -1, j = -1, j2 = -1;
    for (int k = 0; k < 256; ++k) {
      if (!t_cnt[k]) continue;
      if (first < 0) first = k;
      last = k;
      if (t_q[k] <= x) j = k;
      else if (j2 < 0) j2 = k;
    }
    double r;
    if (first < 0) r = (double)v;                            // (an image without pixels: nothing to match to)
    else if (j < 0) r = (double)first;                       // x < xp[0]
    else if (j == last || t_q[j] == x) r = (double)j;
    else r = ((double)(j2 - j) / (t_q[j2] - t_q[j])) * (x - t_q[j]) + (double)j;
    lut[((size_t)b * 3 + ch) * 256 + v] = (float)r;
    __syncthreads();
  }
}

// ---- the spatial ops (MPP_AUG_SPATIAL) --------------------------------------------------------------------------------
// The colour-space round trips run in float64 and round once to float32: a CLAHE bin is round(L* 255 / 100), and a float32
// L* would flip bins that the float64 statement of the op does not.
__device__ __forceinline__ double clip255d(double x) { return fmin(fmax(x, 0.0), 255.0); }

// RandomShadow's pixel: RGB -> HLS (L = (max + min) / 2, hexcone H and S), L *= 0.5, HLS -> RGB
__device__ void shadow_pixel(float x[3]) {
  const double r = (double)x[0] / 255.0, g = (double)x[1] / 255.0, b = (double)x[2] / 255.0;
  const double mx = fmax(r, fmax(g, b)), mn = fmin(r, fmin(g, b)), d = mx - mn;
  const double L = (mx + mn) / 2;
  const double L2 = L * 0.5;
  if (d == 0.0) {
    x[0] = x[1] = x[2] = (float)clip255d(L2 * 255.0);
    return;
  }
  const double S = L < 0.5 ? d / (mx + mn) : d / (2.0 - mx - mn);
  double h;
  if (mx == r) h = (g - b) / d;
  else if (mx == g) h = 2.0 + (b - r) / d;
  else h = 4.0 + (r - g) / d;
  h /= 6.0;
  if (h < 0.0) h += 1.0;
  const double q = L2 <= 0.5 ? L2 * (1.0 + S) : L2 + S - L2 * S, p = 2.0 * L2 - q;
  const double off[3] = {1.0 / 3.0, 0.0, -1.0 / 3.0};
  for (int ch = 0; ch < 3; ++ch) {
    double t = h + off[ch];
    if (t < 0.0) t += 1.0;
    if (t >= 1.0) t -= 1.0;
    double v;
    if (t < 1.0 / 6.0) v = p + (q - p) * 6.0 * t;
    else if (t < 0.5) v = q;
    else if (t < 2.0 / 3.0) v = p + (q - p) * (2.0 / 3.0 - t) * 6.0;
    else v = p;
    x[ch] = (float)clip255d(v * 255.0);
  }
}

// sRGB (gamma, D65) <-> CIE L*a*b* with OpenCV's float constants
__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0; }
__device__ __forceinline__ double lab_finv(double f) { return f > 6.0 / 29.0 ? f * f * f : (f - 16.0 / 116.0) / 7.787; }
__device__ void rgb_to_lab(const float x[3], double lab[3]) {
  double lin[3];
  for (int ch = 0; ch < 3; ++ch) {
    const double c = (double)x[ch] / 255.0;
    lin[ch] = c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4);
  }
  const double X = (0.412453 * lin[0] + 0.357580 * lin[1] + 0.180423 * lin[2]) / 0.950456;
  const double Y = 0.212671 * lin[0] + 0.715160 * lin[1] + 0.072169 * lin[2];
  const double Z = (0.019334 * lin[0] + 0.119193 * lin[1] + 0.950227 * lin[2]) / 1.088754;
  const double fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
  lab[0] = Y > 0.008856 ? 116.0 * fy - 16.0 : 903.3 * Y;
  lab[1] = 500.0 * (fx - fy);
  lab[2] = 200.0 * (fy - fz);
}
__device__ void lab_to_rgb(const double lab[3], float x[3]) {
  const double fy = (lab[0] + 16.0) / 116.0;
  const double Y = lab[0] > 903.3 * 0.008856 ? fy * fy * fy : lab[0] / 903.3;
  const double fy2 = lab_f(Y);                                // (= fy above the knee)
  const double X = lab_finv(lab[1] / 500.0 + fy2) * 0.950456, Z = lab_finv(fy2 - lab[2] / 200.0) * 1.088754;
  const double lin[3] = {3.240479 * X - 1.537150 * Y - 0.498535 * Z, -0.969256 * X + 1.875991 * Y + 0.041556 * Z,
                         0.055648 * X - 0.204043 * Y + 1.057311 * Z};
  for (int ch = 0; ch < 3; ++ch) {
    const double c = lin[ch] <= 0.0031308 ? 12.92 * lin[ch] : 1.055 * pow(lin[ch], 1.0 / 2.4) - 0.055;
    x[ch] = (float)clip255d(c * 255.0);
  }
}
// CLAHE's 8-bit lightness
__device__ __forceinline__ int lab_l8(double L) { return min(255, max(0, (int)rint(L * 255.0 / 100.0))); }

// side of fog's box mean, radius of its discs
__device__ __forceinline__ int fog_hw2(int P, double coef) { return max((int)((double)(P / 3) * coef), 10); }
// BORDER_REFLECT_101
__device__ __forceinline__ int reflect101(int t, int n) { return t < 0 ? -t : (t >= n ? 2 * (n - 1) - t : t); }
// Downscale(0.9), nearest both ways: the source of output index t
__device__ __forceinline__ int down_src(int t, int P) {
  const int d = (int)rint(0.9 * (double)P);
  return min(P - 1, (int)floor((double)(t * d / P) / 0.9));
}
// how many stage outputs k_aug_spatial writes; the last one lies in buffer (n - 1) & 1
__device__ __forceinline__ int spatial_final(const PatchAug &a, int P) {
  const int n = 1 + ((a.fog && fog_hw2(P, a.fog_coef) / 10 > 1) ? 1 : 0) + a.clahe + a.down + (a.blur ? 1 : 0);
  return (n - 1) & 1;
}

__device__ __forceinline__ void swap_ptr(float *&a, float *&b) {
  float *t = a;
  a = b;
  b = t;
}
__device__ __forceinline__ void sort2(float &a, float &b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo;
  b = hi;
}

// One workgroup per patch; ws [B][2][3][P][P] float32.  P % 8 == 0, 32 <= P <= 512 (checked by mpp_train_batch).
__global__ __launch_bounds__(TS) void k_aug_spatial(mpp_train_data data, int P, const int32_t *desc, int flags, uint32_t seed,
                                                    uint32_t epoch, uint32_t batch, const float *lut, float *ws) {
  __shared__ uint32_t hist[64 * 256];              // CLAHE: the 8 x 8 tiles' histograms, then their tables in place
  __shared__ float hm_lut[3][256];
  __shared__ int16_t poly[2][5][2];
  __shared__ int16_t haze[MAXH][2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const Rng g{seed, epoch, batch, (uint32_t)b};
  const PatchAug aug = patch_draws(g, flags, data.n_images);
  if (!aug.spatial()) return;
  const PatchSrc src = patch_src(data, desc, b, P);
  const int PP = P * P;
  float *const base = ws + (size_t)b * 6 * PP;   // the two buffers; a stage reads in and writes out, then they swap
  float *in = base + (size_t)3 * PP, *out = base;

  if (aug.hm)
    for (int k = tid; k < 3 * 256; k += TS) hm_lut[k >> 8][k & 255] = lut[(size_t)b * 768 + k];
  if (aug.shadow && tid < 5 * aug.n_poly) {
    int x, y;
    shadow_vertex(g, P, tid, x, y);
    poly[tid / 5][tid % 5][0] = (int16_t)x;
    poly[tid / 5][tid % 5][1] = (int16_t)y;
  }
  int n_haze = 0;
  if (aug.fog) {
    int x = 0, y = 0;
    n_haze = haze_point(g, P, aug.fog_coef, tid, x, y);
    if (tid < n_haze) {
      haze[tid][0] = (int16_t)x;
      haze[tid][1] = (int16_t)y;
    }
  }
  __syncthreads();

  // stage 1: source, histogram matching, shadow, the fog's discs; without a box mean also the colour ops
  const int hw2 = fog_hw2(P, aug.fog_coef), rad = hw2 / 2, box = aug.fog ? hw2 / 10 : 0;
  const double fog_keep = 1.0 - 0.08 * aug.fog_coef;
  for (int idx = tid; idx < PP; idx += TS) {
    const int i = idx / P, j = idx % P;
    float x[3];
    source_pixel(src, aug, flags, P, i, j, hm_lut, x);
    if (aug.shadow && 2 * i >= P) {
      bool inside = false;
      const double y = (double)i, xq = (double)j;
      for (int m = 0; m < aug.n_poly; ++m) {
        bool c = false;
        int q = 4;
        for (int e = 0; e < 5; ++e) {                // the even-odd rule of csrc/mpp_classics.hpp on the pixel centre
          const double ye = poly[m][e][1], yq = poly[m][q][1], xe = poly[m][e][0], xj = poly[m][q][0];
          if ((((ye <= y) && (y < yq)) || ((yq <= y) && (y < ye))) && (xq < (xj - xe) * (y - ye) / (yq - ye) + xe)) c = !c;
          q = e;
        }
        inside = inside || c;
      }
      if (inside) shadow_pixel(x);
    }
    if (aug.fog) {
      double f = 1.0;
      for (int k = 0; k < n_haze; ++k) {
        const int dx = j - (haze[k][0] + rad), dy = i - (haze[k][1] + rad);
        if (dx * dx + dy * dy <= rad * rad) f = f * fog_keep;
      }
      if (f != 1.0)                                  // v <- 255 alpha + (1 - alpha) v, once per covering disc
        for (int ch = 0; ch < 3; ++ch) x[ch] = (float)clip255d(255.0 - (255.0 - (double)x[ch]) * f);
    }
    if (box <= 1) photometric_color(aug, x);
    for (int ch = 0; ch < 3; ++ch) out[ch * PP + idx] = x[ch];
  }
  swap_ptr(in, out);

  // stage 2: the fog's box mean (side box, anchor box / 2, BORDER_REFLECT_101), then the colour ops
  if (box > 1) {
    __syncthreads();
    const float inv = 1.0f / (float)(box * box);
    for (int idx = tid; idx < PP; idx += TS) {
      const int i = idx / P, j = idx % P;
      float x[3] = {0.f, 0.f, 0.f};
      for (int di = 0; di < box; ++di) {
        const int row = reflect101(i + di - box / 2, P) * P;
        for (int dj = 0; dj < box; ++dj) {
          const int at = row + reflect101(j + dj - box / 2, P);
          for (int ch = 0; ch < 3; ++ch) x[ch] += in[ch * PP + at];
        }
      }
      for (int ch = 0; ch < 3; ++ch) x[ch] = clip255(x[ch] * inv);
      photometric_color(aug, x);
      for (int ch = 0; ch < 3; ++ch) out[ch * PP + idx] = x[ch];
    }
    swap_ptr(in, out);
  }

  // stage 3: CLAHE on the 8-bit lightness
  if (aug.clahe) {
    const int ts = P / 8, area = ts * ts;
    for (int k = tid; k < 64 * 256; k += TS) hist[k] = 0u;
    __syncthreads();
    for (int idx = tid; idx < PP; idx += TS) {
      const int i = idx / P, j = idx % P;
      const float x[3] = {in[idx], in[PP + idx], in[2 * PP + idx]};
      double lab[3];
      rgb_to_lab(x, lab);
      atomicAdd(&hist[((i / ts) * 8 + j / ts) * 256 + lab_l8(lab[0])], 1u);
    }
    __syncthreads();
    // a wave per tile, lane l owns bins 4 l .. 4 l + 3: clip, spread the excess, cumulate, scale
    const int lane = tid & 63;
    const uint32_t limit = (uint32_t)max(1, (int)(aug.clip * (double)area / 256.0));
    for (int tile = tid >> 6; tile < 64; tile += TS / 64) {
      uint32_t *h = hist + tile * 256 + 4 * lane;
      uint32_t v[4], excess = 0u;
      for (int q = 0; q < 4; ++q) {
        v[q] = h[q];
        if (v[q] > limit) {
          excess += v[q] - limit;
          v[q] = limit;
        }
      }
      for (int m = 1; m < 64; m <<= 1) excess += (uint32_t)__shfl_xor((int)excess, m);
      const uint32_t each = excess / 256u, rest = excess % 256u, step = rest ? max(256u / rest, 1u) : 1u;
      uint32_t sum = 0u;
      for (int q = 0; q < 4; ++q) {
        const uint32_t bin = 4u * lane + q;
        v[q] += each + ((rest && bin % step == 0u && bin / step < rest) ? 1u : 0u);
        sum += v[q];
      }
      uint32_t incl = sum;
      for (int m = 1; m < 64; m <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, m);
        if (lane >= m) incl += up;
      }
      uint32_t cum = incl - sum;
      for (int q = 0; q < 4; ++q) {
        cum += v[q];
        h[q] = (uint32_t)min(255, (int)rint((double)cum * 255.0 / (double)area));
      }
    }
    __syncthreads();
    for (int idx = tid; idx < PP; idx += TS) {
      const int i = idx / P, j = idx % P;
      float x[3] = {in[idx], in[PP + idx], in[2 * PP + idx]};
      double lab[3];
      rgb_to_lab(x, lab);
      const int l8 = lab_l8(lab[0]);
      const double tyf = (double)i / (double)ts - 0.5, txf = (double)j / (double)ts - 0.5;
      const int ty = (int)floor(tyf), tx = (int)floor(txf);
      const double ya = tyf - (double)ty, xa = txf - (double)tx;
      const int ty1 = max(ty, 0), ty2 = min(ty + 1, 7), tx1 = max(tx, 0), tx2 = min(tx + 1, 7);
      const double l11 = hist[(ty1 * 8 + tx1) * 256 + l8], l12 = hist[(ty1 * 8 + tx2) * 256 + l8];
      const double l21 = hist[(ty2 * 8 + tx1) * 256 + l8], l22 = hist[(ty2 * 8 + tx2) * 256 + l8];
      const double res = (l11 * (1.0 - xa) + l12 * xa) * (1.0 - ya) + (l21 * (1.0 - xa) + l22 * xa) * ya;
      lab[0] = res * 100.0 / 255.0;
      lab_to_rgb(lab, x);
      for (int ch = 0; ch < 3; ++ch) out[ch * PP + idx] = x[ch];
    }
    swap_ptr(in, out);
  }

  // stage 4: Downscale(0.9), a gather
  if (aug.down) {
    __syncthreads();
    for (int idx = tid; idx < PP; idx += TS) {
      const int at = down_src(idx / P, P) * P + down_src(idx % P, P);
      for (int ch = 0; ch < 3; ++ch) out[ch * PP + idx] = in[ch * PP + at];
    }
    swap_ptr(in, out);
  }

  // stage 5: MedianBlur(3) (BORDER_REPLICATE) or Blur(3) (BORDER_REFLECT_101)
  if (aug.blur) {
    __syncthreads();
    for (int idx = tid; idx < PP; idx += TS) {
      const int i = idx / P, j = idx % P;
      int rows[3], cols[3];
      for (int d = 0; d < 3; ++d) {
        rows[d] = (aug.blur == 1 ? min(max(i + d - 1, 0), P - 1) : reflect101(i + d - 1, P)) * P;
        cols[d] = aug.blur == 1 ? min(max(j + d - 1, 0), P - 1) : reflect101(j + d - 1, P);
      }
      for (int ch = 0; ch < 3; ++ch) {
        float v[9];
        for (int d = 0; d < 9; ++d) v[d] = in[ch * PP + rows[d / 3] + cols[d % 3]];
        float r;
        if (aug.blur == 1) {                        // the median of nine by a 19-exchange network
          sort2(v[1], v[2]); sort2(v[4], v[5]); sort2(v[7], v[8]); sort2(v[0], v[1]); sort2(v[3], v[4]); sort2(v[6], v[7]);
          sort2(v[1], v[2]); sort2(v[4], v[5]); sort2(v[7], v[8]); sort2(v[0], v[3]); sort2(v[5], v[8]); sort2(v[4], v[7]);
          sort2(v[3], v[6]); sort2(v[1], v[4]); sort2(v[2], v[5]); sort2(v[4], v[7]); sort2(v[4], v[2]); sort2(v[6], v[4]);
          sort2(v[4], v[2]);
          r = v[4];
        } else {
          float acc = 0.f;
          for (int d = 0; d < 9; ++d) acc += v[d];
          r = clip255(acc / 9.0f);
        }
        out[ch * PP + idx] = r;
      }
    }
    swap_ptr(in, out);
  }
}

// what patch_draws gives for every patch of a batch, for tests and tools (mpp_train_aug_params)
static_assert(sizeof(mpp_aug_record) == 416, "mpp_aug_record: hip_api.AUG_RECORD_DTYPE restates this layout");
__global__ void k_aug_params(int flags, uint32_t seed, uint32_t epoch, uint32_t batch, int B, int P, int n_images,
                             mpp_aug_record *out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const Rng g{seed, epoch, batch, (uint32_t)b};
  const PatchAug a = patch_draws(g, flags, n_images);
  mpp_aug_record &r = out[b];
  r.rot = a.rot; r.flip = a.flip; r.chan_op = a.chan_op; r.chan_arg = a.chan_arg; r.bc = a.bc; r.color = a.color;
  r.noise = a.noise; r.hm = a.hm; r.tmpl = a.tmpl; r.shadow = a.shadow; r.n_poly = a.n_poly; r.fog = a.fog; r.n_haze = 0;
  r.clahe = a.clahe; r.downscale = a.down; r.blur = a.blur;
  r.alpha = a.alpha; r.beta = a.beta;
  for (int ch = 0; ch < 3; ++ch) r.shift[ch] = a.shift[ch];
  r._pad = 0.f;
  r.sigma = a.sigma; r.blend = a.blend; r.clip = a.clip; r.fog_coef = a.fog_coef;
  for (int v = 0; v < 10; ++v) {
    int x = 0, y = 0;
    if (v < 5 * a.n_poly) shadow_vertex(g, P, v, x, y);
    r.poly[v / 5][v % 5][0] = (int16_t)x;
    r.poly[v / 5][v % 5][1] = (int16_t)y;
  }
  for (int k = 0; k < MAXH; ++k) {
    int x = 0, y = 0;
    const int n = a.fog ? haze_point(g, P, a.fog_coef, k, x, y) : 0;
    if (k == 0) r.n_haze = n;
    r.haze[k][0] = (int16_t)x;
    r.haze[k][1] = (int16_t)y;
  }
}

// SPAT: launched with MPP_AUG_SPATIAL; without it the kernel is compiled as it was before that flag existed
template <bool SPAT>
__global__ __launch_bounds__(TB) void k_train_batch(mpp_train_data data, mpp_train_labels lab, int B, int P, int nb,
                                                    const int32_t *desc, int flags, uint32_t seed, uint32_t epoch,
                                                    uint32_t batch, const float *lut, const float *spat, mpp_train_out out) {
  __shared__ float hm_lut[3][256];                 // the patch's matching table (MPP_AUG_HISTMATCH)
  __shared__ int o_idx[MAXO];              // the object's row in the dataset table
  __shared__ int16_t o_r[MAXO], o_c[MAXO];         // centre in the (transformed) patch
  __shared__ int16_t o_box[MAXO][4];               // rows r0..r1, columns c0..c1 of its polygon's pixels (ShapeNet)
  __shared__ double o_pr[MAXO][4], o_pc[MAXO][4];  // polygon corners (ShapeNet)
  __shared__ uint32_t o_cls[MAXO];                 // its three classes, a byte each (ShapeNet)
  __shared__ int wave_cnt[TB / 64];
  __shared__ double red[TB];

  const int band = blockIdx.x, b = blockIdx.y;
  const Rng g{seed, epoch, batch, (uint32_t)b};
  const PatchAug aug = patch_draws(g, flags, data.n_images);
  // a patch with a spatial op: k_aug_spatial left its image, all but the noise, in the workspace
  const float *fin = SPAT && aug.spatial() ? spat + ((size_t)b * 2 + spatial_final(aug, P)) * 3 * (size_t)P * P : nullptr;
  if (aug.hm && !fin)
    for (int k = threadIdx.x; k < 3 * 256; k += TB) hm_lut[k >> 8][k & 255] = lut[(size_t)b * 768 + k];
  const PatchSrc src = patch_src(data, desc, b, P);
  const int img = desc[3 * b];
  const bool valid = src.valid;
  const int tl_r = src.tl_r, tl_c = src.tl_c;

  // the patch's objects, in annotation order
  int n = 0;
  if (valid) {
    const int s = data.obj_start[img], e = data.obj_start[img + 1];
    for (int base = s; base < e; base += TB) {
      const int i = base + (int)threadIdx.x;
      bool keep = false;
      if (i < e) {
        const int r = data.centers[2 * i] - tl_r, c = data.centers[2 * i + 1] - tl_c;
        keep = r >= 0 && r < P && c >= 0 && c < P;
      }
      int pos;
      const int tot = block_scan(keep, wave_cnt, pos);
      if (keep && n + pos < MAXO) o_idx[n + pos] = i;
      n += tot;
    }
  }
  if (n > MAXO) {
    if (threadIdx.x == 0 && band == 0) atomicMax(out.status, n);
    n = MAXO;
  }
  __syncthreads();
  const bool shape = lab.kind == 1;
  for (int k = threadIdx.x; k < n; k += TB) {
    const int i = o_idx[k];
    int r = data.centers[2 * i] - tl_r, c = data.centers[2 * i + 1] - tl_c;
    double ang = data.params[3 * i + 2];
    if (flags & MPP_AUG_GEOMETRIC) {
      d4_fwd(aug.rot, aug.flip, P, r, c);
      ang = d4_angle(aug.rot, aug.flip, ang);
    }
    o_r[k] = (int16_t)r;
    o_c[k] = (int16_t)c;
    if (shape) {
      const double a = data.params[3 * i], bb = data.params[3 * i + 1];
      const double v[3] = {(a + bb) / 2, a / bb, ang};            // wla_to_sra
      uint32_t d[4] = {0, 0, 0, 0};
      if (flags & MPP_AUG_PERTURB) g.draw(1, (uint32_t)i, d);
      uint32_t packed = 0;
      for (int m = 0; m < 3; ++m) {
        int cl = value_class(lab.edges[m], lab.n_classes, v[m]);
        if (flags & MPP_AUG_PERTURB) {
          const double u = unif(d[m]);
          const int pert = u < 0.8 ? 0 : (u < 0.9 ? 1 : -1);       // {0: 0.8, 1: 0.1, -1: 0.1}
          cl += pert;
          if (lab.cyclic[m]) cl = (cl + lab.n_classes) % lab.n_classes;
          else cl = cl < 0 ? 0 : (cl > lab.n_classes - 1 ? lab.n_classes - 1 : cl);
        }
        packed |= (uint32_t)cl << (8 * m);
      }
      o_cls[k] = packed;
      // rect_to_poly(c, a, b, angle): local corners (+-a/2, +-b/2) @ rot.T + centre
      const double hs = a / 2, hl = bb / 2, cs = cos(ang), sn = sin(ang);
      const double l0[4] = {hs, hs, -hs, -hs}, l1[4] = {hl, -hl, -hl, hl};
      double rmin = 1e300, rmax = -1e300, cmin = 1e300, cmax = -1e300;
      for (int q = 0; q < 4; ++q) {
        const double pr = (l0[q] * cs + l1[q] * (-sn)) + (double)r;
        const double pc = (l0[q] * sn + l1[q] * cs) + (double)c;
        o_pr[k][q] = pr;
        o_pc[k][q] = pc;
        rmin = fmin(rmin, pr); rmax = fmax(rmax, pr); cmin = fmin(cmin, pc); cmax = fmax(cmax, pc);
      }
      // skimage/draw/_draw.pyx _polygon: int(max(0, min)), int(ceil(max)), clipped to the shape
      o_box[k][0] = (int16_t)(int)(rmin > 0.0 ? rmin : 0.0);
      o_box[k][1] = (int16_t)min((int)ceil(rmax), P - 1);
      o_box[k][2] = (int16_t)(int)(cmin > 0.0 ? cmin : 0.0);
      o_box[k][3] = (int16_t)min((int)ceil(cmax), P - 1);
    }
  }
  __syncthreads();

  const int r0 = band * BAND, r1 = min(P, r0 + BAND);
  const size_t PP = (size_t)P * P;
  double cnt = 0.0, sdil = 0.0;
  for (int idx = threadIdx.x; idx < (r1 - r0) * P; idx += TB) {
    const int i = r0 + idx / P, j = idx % P;
    const size_t px = (size_t)b * PP + (size_t)i * P + j;
    float x[3];
    if (fin) {
      for (int ch = 0; ch < 3; ++ch) x[ch] = fin[(size_t)ch * PP + (size_t)i * P + j];
      photometric_noise(aug, g, i * P + j, x);
    } else {
      source_pixel(src, aug, flags, P, i, j, hm_lut, x);
      if (flags & (MPP_AUG_MEDIUM | MPP_AUG_STRONG)) photometric(aug, g, i * P + j, x);
    }
    for (int ch = 0; ch < 3; ++ch) out.patch[((size_t)b * 3 + ch) * PP + (size_t)i * P + j] = x[ch] / 255.0f;

    if (!shape) {
      int best = 0x7fffffff, arg = -1;
      for (int k = 0; k < n; ++k) {
        const int dr = o_r[k] - i, dc = o_c[k] - j;
        const int d2 = dr * dr + dc * dc;
        if (d2 < best) { best = d2; arg = k; }
      }
      // scipy's distance_transform_edt of a map without a zero measures from (-1, 0)
      if (arg < 0) best = (i + 1) * (i + 1) + j * j;
      const double dist = sqrt((double)best);
      const double t = dist / lab.sigma_dil;
      double dil = exp(-0.5 * (t * t));
      if (dil < 1e-5) dil = 0.0;
      double vr = 0.0, vc = 0.0;
      bool in = false;
      if (arg >= 0) {
        vr = (double)(o_r[arg] - i);
        vc = (double)(o_c[arg] - j);
        const double norm = sqrt(vr * vr + vc * vc) + 1e-8;
        if (lab.uvec) { vr = vr / norm; vc = vc / norm; }
        in = !(norm > lab.max_distance);
        if (!in) vr = vc = 0.0;
      }
      const float fdil = (float)dil;
      if (out.vec) {
        out.vec[((size_t)b * 2) * PP + (size_t)i * P + j] = (float)vr;
        out.vec[((size_t)b * 2 + 1) * PP + (size_t)i * P + j] = (float)vc;
      }
      if (out.mask) out.mask[px] = in ? 1.f : 0.f;
      if (out.dil) out.dil[px] = fdil;
      if (out.dist) out.dist[px] = (float)dist;
      cnt += in ? 1.0 : 0.0;
      sdil += (double)fdil;
    } else {
      uint32_t cls = 0;
      bool cov = false;
      const double y = (double)i, xq = (double)j;
      for (int k = 0; k < n; ++k) {
        if (i < o_box[k][0] || i > o_box[k][1] || j < o_box[k][2] || j > o_box[k][3]) continue;
        bool c = false;
        int q = 3;
        for (int e = 0; e < 4; ++e) {                // _point_in_polygon(xp = cols, yp = rows, x = j, y = i)
          const double ye = o_pr[k][e], yq = o_pr[k][q], xe = o_pc[k][e], xj = o_pc[k][q];
          if ((((ye <= y) && (y < yq)) || ((yq <= y) && (y < ye))) && (xq < (xj - xe) * (y - ye) / (yq - ye) + xe)) c = !c;
          q = e;
        }
        if (c) { cov = true; cls = o_cls[k]; }
      }
      if (out.cls)
        for (int m = 0; m < 3; ++m) out.cls[((size_t)m * B) * PP + px] = (uint8_t)(cls >> (8 * m));
      if (out.cover) out.cover[px] = cov ? 1 : 0;
      cnt += cov ? 1.0 : 0.0;
    }
  }
  const double c_tot = block_sum(cnt, red), d_tot = block_sum(sdil, red);
  if (threadIdx.x == 0) {
    out.sums[((size_t)b * nb + band) * 2] = c_tot;
    out.sums[((size_t)b * nb + band) * 2 + 1] = d_tot;
  }
}

// partials of this workgroup -> ws; the last workgroup reduces them in order and writes res[q] (q < nv) and the total
// res[3] = res[0] + res[1] + res[2]
__device__ void finish(double *part, unsigned *done, int nparts, const double *v, int nv, double *res, double *red) {
  __shared__ int last;
  const int blk = blockIdx.x + blockIdx.y * gridDim.x;
  if (threadIdx.x == 0) {
    for (int q = 0; q < nv; ++q) part[(size_t)blk * 8 + q] = v[q];
    __threadfence();
    last = atomicAdd(done, 1u) == (unsigned)(nparts - 1);
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  for (int q = 0; q < nv; ++q) {
    double acc = 0.0;
    for (int p = threadIdx.x; p < nparts; p += TB) acc += __builtin_nontemporal_load(&part[(size_t)p * 8 + q]);
    const double t = block_sum(acc, red);
    if (threadIdx.x == 0) res[q] = t;
  }
  if (threadIdx.x == 0) {
    res[3] = res[0] + res[1] + res[2];
    *done = 0u;
  }
}

// both betas of the batch from the band sums of mpp_train_batch (fixed order: the same in every workgroup)
__device__ void batch_sums(const double *sums, int nrows, double *red, double &s0, double &s1) {
  double a = 0.0, c = 0.0;
  for (int p = threadIdx.x; p < nrows; p += TB) {
    a += sums[2 * p];
    c += sums[2 * p + 1];
  }
  s0 = block_sum(a, red);
  s1 = block_sum(c, red);
}

// The reference runs these losses in float32, and where a sigmoid saturates its value is float32 arithmetic: 1 - sigmoid(x)
// is exactly 0 above x ~ 17, so log(1 - q + eps) is log(eps) and the sigmoid's backward (1 - y) * y is 0.  So the sigmoids,
// the divergence and the arguments of the logs are formed in float32 as torch forms them (sigmf, div_at: mpp_unet_math.hpp, the
// functions of the inference epilogues); the rest, and every sum, is float64.
// balanced BCE of a float32 sigmoid output y against target t: the loss term and dL/dy
__device__ __forceinline__ void bce(float y, double t, double beta, double &loss, double &dy) {
  const double la = (double)(y + 1e-5f), lb = (double)((1.0f - y) + 1e-5f);
  loss = -beta * t * log(la) - (1.0 - beta) * (1.0 - t) * log(lb);
  dy = -beta * t / la + (1.0 - beta) * (1.0 - t) / lb;
}
// dL/dz at a pixel (z -> q -> BCE against dil, / N)
__device__ __forceinline__ double dz_at(const DivAt &d, double y, double beta, double invN) {
  double l, dq;
  bce(d.q, y, beta, l, dq);
  return invN * dq * (double)d.q * (double)(1.0f - d.q);
}

__global__ __launch_bounds__(TB) void k_posnet_loss(int B, int P, int nb, const float *out, const float *vec, const float *mask,
                                                    const float *dil, const double *sums, int with_div, const float *wp,
                                                    const float *bp, float *grad, double *part, unsigned *done, double *res) {
  __shared__ double red[TB];
  const int band = blockIdx.x, b = blockIdx.y;
  const size_t PP = (size_t)P * P;
  const double N = (double)B * (double)PP, invN = 1.0 / N;
  double smask, sdil;
  batch_sums(sums, B * nb, red, smask, sdil);
  // beta = 1 - sum(target) / numel: the targets are float32 maps summed by torch in float32
  const double beta_m = 1.0 - (double)(float)smask / N, beta_d = 1.0 - (double)(float)sdil / N;
  const float w = with_div ? wp[0] : 0.f, bias = with_div ? bp[0] : 0.f;
  const float *o = out + (size_t)b * 3 * PP;
  const float *t = vec + (size_t)b * 2 * PP;
  __builtin_assume(P >= 3);                 // (mpp_posnet_loss checks it: grad1's one-element case is never reached)
  auto px = [&](int i, int j, int ch) -> float { return o[ch * PP + (size_t)i * P + j]; };   // the patch's [3][P][P] output
  double acc[5] = {0, 0, 0, 0, 0};          // vec, mask, div losses (sums), dL/dw, dL/db
  const int r0 = band * BAND, r1 = min(P, r0 + BAND);
  for (int idx = threadIdx.x; idx < (r1 - r0) * P; idx += TB) {
    const int i = r0 + idx / P, j = idx % P;
    const size_t pix = (size_t)i * P + j;
    const float sf = sigmf(o[2 * PP + pix]);
    const double o0 = o[pix], o1 = o[PP + pix], s = sf;
    const double e0 = o0 * s - (double)t[pix], e1 = o1 * s - (double)t[PP + pix];
    acc[0] += e0 * e0 + e1 * e1;
    const double m = mask[(size_t)b * PP + pix];
    double lm, dsm;
    bce(sf, m, beta_m, lm, dsm);
    acc[1] += lm;
    double ds = (e0 * o0 + e1 * o1) * invN + dsm * invN;                  // vec_loss = mean over B*2*P*P
    double g0 = e0 * s * invN, g1 = e1 * s * invN;
    if (with_div) {
      const DivAt d = div_at(px, i, j, P, P, w, bias);
      const double y = dil[(size_t)b * PP + pix];
      double ld, dq;
      bce(d.q, y, beta_d, ld, dq);
      acc[2] += ld;
      const double dz = invN * dq * (double)d.q * (double)(1.0f - d.q);
      acc[3] += dz * (double)d.x;
      acc[4] += dz;
      ds += dz * (double)w * (double)d.div;
      // adjoint of the stencils: h = dL/d(div) = dz * w * s at the pixels whose divergence reads this one
      auto h = [&](int ii, int jj) {
        const DivAt e = div_at(px, ii, jj, P, P, w, bias);
        return dz_at(e, dil[(size_t)b * PP + (size_t)ii * P + jj], beta_d, invN) * (double)w * (double)e.s;
      };
      // rows (channel 0): g[0] = f1 - f0, g[n-1] = f[n-1] - f[n-2], g[k] = (f[k+1] - f[k-1]) / 2
      double a0 = 0.0, a1 = 0.0;
      if (i == 0) a0 -= h(0, j);
      if (i == 1) a0 += h(0, j);
      if (i == P - 1) a0 += h(P - 1, j);
      if (i == P - 2) a0 -= h(P - 1, j);
      if (i - 1 >= 1 && i - 1 <= P - 2) a0 += 0.5 * h(i - 1, j);
      if (i + 1 >= 1 && i + 1 <= P - 2) a0 -= 0.5 * h(i + 1, j);
      if (j == 0) a1 -= h(i, 0);
      if (j == 1) a1 += h(i, 0);
      if (j == P - 1) a1 += h(i, P - 1);
      if (j == P - 2) a1 -= h(i, P - 1);
      if (j - 1 >= 1 && j - 1 <= P - 2) a1 += 0.5 * h(i, j - 1);
      if (j + 1 >= 1 && j + 1 <= P - 2) a1 -= 0.5 * h(i, j + 1);
      g0 += a0;
      g1 += a1;
    }
    if (grad) {
      float *gp = grad + (size_t)b * 3 * PP;
      gp[pix] = (float)g0;
      gp[PP + pix] = (float)g1;
      gp[2 * PP + pix] = (float)(ds * s * (double)(1.0f - sf));
    }
  }
  double v[6];
  v[0] = block_sum(acc[0], red) / (2.0 * N);
  v[1] = block_sum(acc[1], red) / N;
  v[2] = block_sum(acc[2], red) / N;
  v[3] = 0.0;
  v[4] = block_sum(acc[3], red);
  v[5] = block_sum(acc[4], red);
  finish(part, done, gridDim.x * gridDim.y, v, 6, res, red);
}

__global__ __launch_bounds__(TB) void k_shapenet_loss(int B, int P, int nb, int nc, const float *l0, const float *l1,
                                                      const float *l2, const uint8_t *cls, const uint8_t *cover,
                                                      const double *sums, float *g0, float *g1, float *g2, double *part,
                                                      unsigned *done, double *res) {
  __shared__ double red[TB];
  __shared__ double cnt_s;
  const int band = blockIdx.x, b = blockIdx.y;
  const size_t PP = (size_t)P * P;
  if (threadIdx.x == 0) {
    double c = 0.0;
    for (int q = 0; q < nb; ++q) c += sums[((size_t)b * nb + q) * 2];
    cnt_s = c;
  }
  __syncthreads();
  const double cnt = cnt_s;
  const double invB = 1.0 / (double)B;
  const float *L[3] = {l0, l1, l2};
  float *G[3] = {g0, g1, g2};
  double acc[3] = {0, 0, 0};
  const int r0 = band * BAND, r1 = min(P, r0 + BAND);
  for (int idx = threadIdx.x; idx < (r1 - r0) * P; idx += TB) {
    const int i = r0 + idx / P, j = idx % P;
    const size_t pix = (size_t)i * P + j, px = (size_t)b * PP + pix;
    const double wgt = cover[px] ? 1.0 / cnt : 0.0;          // loss_mask: the union / its count (0 for an empty patch)
    for (int h = 0; h < 3; ++h) {
      const size_t base = (size_t)b * nc * PP + pix;
      if (wgt == 0.0) {                                       // nothing to read: the pixel's loss and gradient are 0
        if (G[h])
          for (int c = 0; c < nc; ++c) G[h][base + (size_t)c * PP] = 0.f;
        continue;
      }
      const float *x = L[h] + base;
      float mx = -INFINITY;
      for (int c = 0; c < nc; ++c) mx = fmaxf(mx, x[(size_t)c * PP]);
      double se = 0.0;
      for (int c = 0; c < nc; ++c) se += exp((double)x[(size_t)c * PP] - (double)mx);
      const int y = cls[((size_t)h * B) * PP + px];
      const double lse = log(se) + (double)mx;
      acc[h] += (lse - (double)x[(size_t)y * PP]) * wgt;
      if (G[h]) {
        const double gs = wgt * invB;
        for (int c = 0; c < nc; ++c) {
          const double p = exp((double)x[(size_t)c * PP] - lse);
          G[h][base + (size_t)c * PP] = (float)((p - (c == y ? 1.0 : 0.0)) * gs);
        }
      }
    }
  }
  double v[3];
  for (int h = 0; h < 3; ++h) v[h] = block_sum(acc[h], red) * invB;
  finish(part, done, gridDim.x * gridDim.y, v, 3, res, red);
}

}  // namespace

hipError_t mpp_train_ws_reserve(TrainWs *ws, size_t workgroups) {
  if (!ws->done) {
    hipError_t e = hipMalloc((void **)&ws->done, sizeof(unsigned));
    if (e != hipSuccess) return e;
    e = hipMemset(ws->done, 0, sizeof(unsigned));
    if (e != hipSuccess) return e;
  }
  if (ws->part_count < workgroups) {
    if (ws->part) (void)hipFree(ws->part);
    ws->part = nullptr;
    ws->part_count = 0;
    hipError_t e = hipMalloc((void **)&ws->part, workgroups * 8 * sizeof(double));
    if (e != hipSuccess) return e;
    ws->part_count = workgroups;
  }
  return hipSuccess;
}

void mpp_train_ws_free(TrainWs *ws) {
  if (ws->part) (void)hipFree(ws->part);
  if (ws->done) (void)hipFree(ws->done);
  if (ws->lut) (void)hipFree(ws->lut);
  if (ws->spat) (void)hipFree(ws->spat);
  ws->spat = nullptr;
  ws->spat_floats = 0;
  ws->part = nullptr;
  ws->done = nullptr;
  ws->lut = nullptr;
  ws->part_count = 0;
  ws->lut_patches = 0;
}

hipError_t mpp_launch_train_batch(hipStream_t st, TrainWs *ws, const mpp_train_data &data, const mpp_train_labels &labels,
                                  int B, int P, const int32_t *desc, int flags, uint32_t seed, uint32_t epoch, uint32_t batch,
                                  const mpp_train_out &out) {
  const int nb = (P + BAND - 1) / BAND;
  if (flags & MPP_AUG_HISTMATCH) {
    if (ws->lut_patches < (size_t)B) {
      if (ws->lut) (void)hipFree(ws->lut);
      ws->lut = nullptr;
      ws->lut_patches = 0;
      hipError_t e = hipMalloc((void **)&ws->lut, (size_t)B * 768 * sizeof(float));
      if (e != hipSuccess) return e;
      ws->lut_patches = (size_t)B;
    }
    hipLaunchKernelGGL(k_hist_lut, dim3(B), dim3(TB), 0, st, data, P, desc, ws->hist, seed, epoch, batch, ws->lut);
  }
  if (flags & MPP_AUG_SPATIAL) {
    const size_t need = (size_t)B * 6 * P * P;              // a ping-pong pair of float32 patches per patch
    if (ws->spat_floats < need) {
      if (ws->spat) (void)hipFree(ws->spat);
      ws->spat = nullptr;
      ws->spat_floats = 0;
      hipError_t e = hipMalloc((void **)&ws->spat, need * sizeof(float));
      if (e != hipSuccess) return e;
      ws->spat_floats = need;
    }
    hipLaunchKernelGGL(k_aug_spatial, dim3(B), dim3(TS), 0, st, data, P, desc, flags, seed, epoch, batch,
                       (const float *)ws->lut, ws->spat);
  }
  if (flags & MPP_AUG_SPATIAL)
    hipLaunchKernelGGL(k_train_batch<true>, dim3(nb, B), dim3(TB), 0, st, data, labels, B, P, nb, desc, flags, seed, epoch,
                       batch, (const float *)ws->lut, (const float *)ws->spat, out);
  else
    hipLaunchKernelGGL(k_train_batch<false>, dim3(nb, B), dim3(TB), 0, st, data, labels, B, P, nb, desc, flags, seed, epoch,
                       batch, (const float *)ws->lut, (const float *)nullptr, out);
  return hipGetLastError();
}

hipError_t mpp_launch_aug_params(hipStream_t st, int flags, uint32_t seed, uint32_t epoch, uint32_t batch, int B, int P,
                                 int n_images, mpp_aug_record *out) {
  hipLaunchKernelGGL(k_aug_params, dim3((B + 63) / 64), dim3(64), 0, st, flags, seed, epoch, batch, B, P, n_images, out);
  return hipGetLastError();
}

hipError_t mpp_launch_posnet_loss(hipStream_t st, TrainWs *ws, int B, int P, const float *out, const float *vec,
                                  const float *mask, const float *dil, const double *sums, int with_div, const float *w,
                                  const float *b, float *grad, double *res) {
  const int nb = (P + BAND - 1) / BAND;
  hipError_t e = mpp_train_ws_reserve(ws, (size_t)nb * B);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_posnet_loss, dim3(nb, B), dim3(TB), 0, st, B, P, nb, out, vec, mask, dil, sums, with_div, w, b, grad,
                     ws->part, ws->done, res);
  return hipGetLastError();
}

hipError_t mpp_launch_shapenet_loss(hipStream_t st, TrainWs *ws, int B, int P, int n_classes, const float *l0,
                                    const float *l1, const float *l2, const uint8_t *cls, const uint8_t *cover,
                                    const double *sums, float *g0, float *g1, float *g2, double *res) {
  const int nb = (P + BAND - 1) / BAND;
  hipError_t e = mpp_train_ws_reserve(ws, (size_t)nb * B);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_shapenet_loss, dim3(nb, B), dim3(TB), 0, st, B, P, nb, n_classes, l0, l1, l2, cls, cover, sums, g0, g1,
                     g2, ws->part, ws->done, res);
  return hipGetLastError();
}
