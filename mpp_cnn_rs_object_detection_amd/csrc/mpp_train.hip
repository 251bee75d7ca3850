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
//  * k_posnet_loss / k_shapenet_loss: one workgroup per (patch, band); each writes the loss and dL/dout of its pixels and
//    its partial sums, and the last workgroup to finish reduces the partials in a fixed order (the same inputs give the
//    same bits).
//
// Random draws: Philox4x32-10, key (seed, epoch), counter (batch, patch, stream, index); stream 0: the patch's draws,
// 1: class perturbation of an object (index: its row in the dataset's object table), 2: pixel noise (index: pixel).
// Stream 0's indices: 0 D4, 1..4 the photometric ops, 5 histogram matching.
#include <cmath>
#include <cstdint>

#include "mpp_device.hpp"
#include "mpp_train.hpp"

namespace {

constexpr int TB = 256;                    // threads of every workgroup here
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
// composed as data/augmentation.py:22-72 lays them out; CLAHE, shadow, fog, downscale and blur are not built
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
    a.color = w < 0.5 ? 0 : (w < 1.0 ? 1 : 2);            // 0: CLAHE, not built
  }
  g.draw(0, 3, d);
  for (int ch = 0; ch < 3; ++ch) a.shift[ch] = (float)(unif(d[ch]) * 40.0 - 20.0);
  a.noise = unif(d[3]) < 0.5;                              // GaussNoise()
  g.draw(0, 4, d);
  a.sigma = sqrt(10.0 + unif(d[0]) * 40.0);
  return a;
}

__device__ void photometric(const PatchAug &a, const Rng &g, int pix, float x[3]) {
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
  if (a.noise) {
    uint32_t d[4];
    g.draw(2, (uint32_t)pix, d);
    const double r0 = sqrt(-2.0 * log(unif(d[0]))), r1 = sqrt(-2.0 * log(unif(d[2])));
    const double t0 = 2.0 * PI * unif(d[1]), t1 = 2.0 * PI * unif(d[3]);
    const double z[3] = {r0 * cos(t0), r0 * sin(t0), r1 * cos(t1)};
    for (int ch = 0; ch < 3; ++ch) x[ch] = clip255((float)((double)x[ch] + a.sigma * z[ch]));
  }
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

__global__ __launch_bounds__(TB) void k_train_batch(mpp_train_data data, mpp_train_labels lab, int B, int P, int nb,
                                                    const int32_t *desc, int flags, uint32_t seed, uint32_t epoch,
                                                    uint32_t batch, const float *lut, mpp_train_out out) {
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
  if (aug.hm)
    for (int k = threadIdx.x; k < 3 * 256; k += TB) hm_lut[k >> 8][k & 255] = lut[(size_t)b * 768 + k];
  const int img = desc[3 * b];
  const bool valid = img >= 0 && img < data.n_images;
  const int tl_r = desc[3 * b + 1] - P / 2, tl_c = desc[3 * b + 2] - P / 2;
  const int H = valid ? data.img_hw[2 * img] : 0, W = valid ? data.img_hw[2 * img + 1] : 0;
  const uint8_t *im = valid ? data.images + data.img_off[img] : nullptr;

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
    // the patch: a read at tl + (source pixel), zeros outside the image
    int si = i, sj = j;
    if (flags & MPP_AUG_GEOMETRIC) d4_inv(aug.rot, aug.flip, P, si, sj);
    const int gr = tl_r + si, gc = tl_c + sj;
    float x[3] = {0.f, 0.f, 0.f};
    if (valid && gr >= 0 && gr < H && gc >= 0 && gc < W) {
      const uint8_t *p = im + ((size_t)gr * W + gc) * 3;
      x[0] = (float)p[0]; x[1] = (float)p[1]; x[2] = (float)p[2];
    }
    if (aug.hm)                                               // one rounding: the blend is formed in float64
      for (int ch = 0; ch < 3; ++ch)
        x[ch] = clip255((float)(aug.blend * (double)hm_lut[ch][(int)x[ch]] + (1.0 - aug.blend) * (double)x[ch]));
    if (flags & (MPP_AUG_MEDIUM | MPP_AUG_STRONG)) photometric(aug, g, i * P + j, x);
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
// the divergence and the arguments of the logs are formed in float32 as torch forms them; the rest, and every sum, is float64.
__device__ __forceinline__ float sigmf(float x) { return 1.0f / (1.0f + expf(-x)); }

// the divergence classifier at (i, j): div = d(out0)/drow + d(out1)/dcol (torch.gradient: one-sided at the edges, central
// inside), x = div * sigmoid(out2), z = w x + b, q = sigmoid(z)
struct DivAt { float div, s, x, q; };
__device__ __forceinline__ float grad1(const float *f, int n, int stride, int i) {
  if (i == 0) return f[stride] - f[0];
  if (i == n - 1) return f[(size_t)(n - 1) * stride] - f[(size_t)(n - 2) * stride];
  return (f[(size_t)(i + 1) * stride] - f[(size_t)(i - 1) * stride]) / 2.0f;
}
__device__ __forceinline__ DivAt div_at(const float *o, size_t PP, int P, int i, int j, float w, float bias) {
  DivAt d;
  d.div = grad1(o + j, P, P, i) + grad1(o + PP + (size_t)i * P, P, 1, j);
  d.s = sigmf(o[2 * PP + (size_t)i * P + j]);
  d.x = d.div * d.s;
  d.q = sigmf(w * d.x + bias);
  return d;
}
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
      const DivAt d = div_at(o, PP, P, i, j, w, bias);
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
        const DivAt e = div_at(o, PP, P, ii, jj, w, bias);
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
  hipLaunchKernelGGL(k_train_batch, dim3(nb, B), dim3(TB), 0, st, data, labels, B, P, nb, desc, flags, seed, epoch, batch,
                     (const float *)ws->lut, out);
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
