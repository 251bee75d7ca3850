// mpp_prepass.hip -- the birth pre-pass of a deep launch (table layout: mpp_prepass.hpp).
//
// Three kernels on the launch's stream, one thread per step of every chain of the launch:
//   count  kernel type of each step (Philox block 0), births per block of PRE_BLOCK steps;
//   scan   the births' ordinals: exclusive prefix of the block counts over all chains (one workgroup);
//   fill   per step its word (type | ordinal, or type | queue position), per birth its record: draw_head / draw_birth (lane forms), deep_add_geo and
//          deep_pre -- the very functions the deep kernel ran for a birth lane, so the record holds its bits.
// The host reads the number of births back between scan and fill (the records' size; a table over the prepass_mb budget
// is not built and the launch draws its births itself).
// With the queues (qcnt / qoff non-null) count also counts every type per block, a second scan -- one workgroup per chain --
// turns those counts into queue positions, and fill writes every step's queue entry: the head of its proposal
// (draw_head_q), or, for a birth, its ordinal in the records.
#include "mpp_chain.hpp"
#include "mpp_prepass.hpp"
#include "mpp_launch.hpp"

// the Philox key of chain `tile`, formed as the chain kernels form it (mpp_deep.hip, mpp_chain_body.inc)
__device__ __forceinline__ void pre_key(const TileRef &t, unsigned long long seed, uint32_t chain0, int tile, uint32_t *k0,
                                        uint32_t *k1, uint32_t *chain) {
  const unsigned long long seed_t = t.key_on ? (unsigned long long)t.key_seed : seed;
  *chain = t.key_on ? t.key_chain : chain0 + (uint32_t)tile;
  *k0 = (uint32_t)seed_t; *k1 = (uint32_t)(seed_t >> 32);
}
__device__ __forceinline__ int pre_type(const DevParams *P, uint32_t a, uint32_t b) {
  const double uk = u53(a, b);
  int kt = 0;
  while (kt < P->n_kernels - 1 && P->p_cum[kt] <= uk) ++kt;
  return kt;
}
__device__ __forceinline__ bool is_birth(int kt) { return kt == MPP_K_UBIRTH || kt == MPP_K_DBIRTH; }

// grid (blocks of steps, chains)
__global__ __launch_bounds__(PRE_BLOCK) void mpp_prepass_count_kernel(const DevParams Pv, const TileRef *tiles, int tile0,
                                                                      const long long *until, unsigned long long seed,
                                                                      unsigned int chain0, int nblk, long long stride,
                                                                      unsigned int *cnt, unsigned int *qcnt) {
  const int ch = blockIdx.y, tile = tile0 + ch;
  const TileRef t = tiles[tile];
  const long long rel = (long long)blockIdx.x * PRE_BLOCK + threadIdx.x, s = *t.step + rel;
  int kt = 15;
  if (s < until[tile] && rel < stride) {
    uint32_t k0, k1, chain, w[4];
    pre_key(t, seed, chain0, tile, &k0, &k1, &chain);
    philox4x32_10((uint32_t)s, (uint32_t)((uint64_t)s >> 32), 0u, chain, k0, k1, w);
    kt = pre_type(&Pv, w[0], w[1]);
  }
  const int c = __syncthreads_count(is_birth(kt));
  if (threadIdx.x == 0) cnt[(size_t)ch * nblk + blockIdx.x] = (unsigned int)c;
  if (qcnt) {
    for (int k = 0; k < MPP_NKERNEL; ++k) {
      const int ck = __syncthreads_count(kt == k);
      if (threadIdx.x == 0) qcnt[((size_t)ch * MPP_NKERNEL + k) * nblk + blockIdx.x] = (unsigned int)ck;
    }
  }
}

// in place: cnt[i] <- sum of cnt[0 .. i-1]; *total <- sum of all -- for each of the grid's segments of n counts
__global__ __launch_bounds__(1024) void mpp_prepass_scan_kernel(unsigned int *cnt, long long n, unsigned long long *total) {
  __shared__ unsigned long long part[1024];
  const int tid = threadIdx.x;
  cnt += (size_t)blockIdx.x * n;
  total += blockIdx.x;
  unsigned long long carry = 0;
  for (long long i0 = 0; i0 < n; i0 += 1024) {
    const long long i = i0 + tid;
    const unsigned long long v = i < n ? cnt[i] : 0u;
    part[tid] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const unsigned long long x = tid >= off ? part[tid - off] : 0ull;
      __syncthreads();
      part[tid] += x;
      __syncthreads();
    }
    if (i < n) cnt[i] = (unsigned int)(carry + part[tid] - v);
    carry += part[1023];
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// grid (blocks of steps, chains); off: the scanned block counts
__global__ __launch_bounds__(PRE_BLOCK) void mpp_prepass_fill_kernel(const DevParams Pv, const TileRef *tiles, int tile0,
                                                                     const long long *until, unsigned long long seed,
                                                                     unsigned int chain0, int nblk, long long stride,
                                                                     const unsigned int *off, uint32_t *word, double *rec,
                                                                     const unsigned int *qcnt, uint32_t *qoff, QEnt *qent,
                                                                     long long *base) {
  __shared__ double s_edges[3 * MPP_NCLASS];
  __shared__ unsigned int s_wcnt[PRE_BLOCK / WAVE];
  __shared__ unsigned int s_tcnt[PRE_BLOCK / WAVE][MPP_NKERNEL];
  const DevParams *P = &Pv;
  const int ch = blockIdx.y, tile = tile0 + ch, tid = threadIdx.x;
  for (int i = tid; i < 3 * MPP_NCLASS; i += PRE_BLOCK) s_edges[i] = P->maps.edges[i / MPP_NCLASS][i % MPP_NCLASS];
  Chain c;
  c.P = P; c.t = tiles[tile];
  load_hot(c);
  c.L = Lds{};
  c.L.edges = s_edges;          // (what the chain copies to LDS; the birth CDF's row level is read from the tile: same values)
  c.L.rowbase = nullptr;
  c.lane = tid & (WAVE - 1);
  c.wave = tid / WAVE;
  const long long s0 = *c.t.step, rel = (long long)blockIdx.x * PRE_BLOCK + tid, s = s0 + rel;
  const bool in = s < until[tile] && rel < stride;
  if (base && blockIdx.x == 0 && tid == 0) base[ch] = s0;
  uint32_t k0, k1, chain, w[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  pre_key(c.t, seed, chain0, tile, &k0, &k1, &chain);
  int kt = 15;
  if (in) {
    philox4x32_10((uint32_t)s, (uint32_t)((uint64_t)s >> 32), 0u, chain, k0, k1, w);
    kt = pre_type(P, w[0], w[1]);
  }
  const bool birth = in && is_birth(kt);
  // the births' ordinals in step order: the block's base, then the waves before mine, then the lanes before mine
  const unsigned long long m = __ballot(birth);
  if (c.lane == 0) s_wcnt[c.wave] = (unsigned int)__popcll(m);
  __syncthreads();
  unsigned int ord = off[(size_t)ch * nblk + blockIdx.x] + (unsigned int)__popcll(m & ((1ull << c.lane) - 1ull));
  for (int v = 0; v < c.wave; ++v) ord += s_wcnt[v];
  uint32_t wd = (uint32_t)kt | (birth ? ord << 4 : 0u);
  if (qoff) {
    // my position in my type's queue: the block's first, then the waves before mine, then the lanes before mine
    unsigned long long same = 0ull;
    unsigned int cnt_lane = 0;
#pragma unroll
    for (int k = 0; k < MPP_NKERNEL; ++k) {
      const unsigned long long mk = __ballot(kt == k);
      if (kt == k) same = mk;
      if (c.lane == k) cnt_lane = (unsigned int)__popcll(mk);
    }
    if (c.lane < MPP_NKERNEL) s_tcnt[c.wave][c.lane] = cnt_lane;
    __syncthreads();
    if (in) {
      unsigned int pos = qcnt[((size_t)ch * MPP_NKERNEL + kt) * nblk + blockIdx.x] + (unsigned int)__popcll(same & ((1ull << c.lane) - 1ull));
      for (int v = 0; v < c.wave; ++v) pos += s_tcnt[v][kt];
      QEnt e;
      e.off = (uint32_t)rel; e.w2 = ord; e.u_acc = 0.0; e.a = 0.0; e.b = 0.0;
      if (!birth) {
        philox4x32_10((uint32_t)s, (uint32_t)((uint64_t)s >> 32), 1u, chain, k0, k1, w + 4);
        draw_head_q(P, kt, w, e);
      }
      const size_t at = (size_t)ch * stride + pos;
      qoff[at] = (uint32_t)rel;
      qent[at] = e;
      // step to entry: the hot start (mpp_hot.hip) looks a step up by its index, so the word of a step that is no birth
      // carries its queue position where a birth's carries its ordinal (28 bits)
      if (!birth && stride < (1ll << 28)) wd |= pos << 4;
    }
  }
  if (in) word[(size_t)ch * stride + rel] = wd;
  if (!birth) return;
  philox4x32_10((uint32_t)s, (uint32_t)((uint64_t)s >> 32), 1u, chain, k0, k1, w + 4);
  Rec r;
  r.valid = 1; r.accepted = 0; r._pad = 0; r.n_stash = 0; r.gate_a = 1;
  const int k = draw_head<true>(c, w, r, k0, k1, (uint64_t)s, chain);
  int keep = 0;
  MapVals pmv{0.f, 0.f, 0.f, 0.f, 0.0, 0.0, 0.0, 0};
  draw_birth<true>(c, w, k, r, &keep, &pmv);
  deep_add_geo(c, r, keep);
  deep_pre<false>(c, r, keep, false, pmv, nullptr);
  double2 *o = (double2 *)(rec + (size_t)ord * PRE_REC_DOUBLES);
  const unsigned long long bits = (unsigned long long)((unsigned int)(r.ax & 0xffff) | ((unsigned int)r.ay << 16)) |
                                  ((unsigned long long)(unsigned int)r.gate_a << 32);
  o[0] = make_double2(r.u_acc, r.qf);
  o[1] = make_double2(r.as, r.ar);
  o[2] = make_double2(r.aa, r.lin_a);
  o[3] = make_double2(r.hl, r.hw);
  o[4] = make_double2(r.ca, r.sa);
  o[5] = make_double2(r.rad, __longlong_as_double((long long)bits));
}

// ---- host-side launchers ----------------------------------------------------------------------------
extern "C" hipError_t mpp_prepass_count(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile0, int n_chains,
                                        const long long *until, unsigned long long seed, unsigned int chain0, int nblk,
                                        long long stride, unsigned int *cnt, unsigned long long *total, unsigned int *qcnt,
                                        unsigned long long *qtot) {
  hipLaunchKernelGGL(mpp_prepass_count_kernel, dim3(nblk, n_chains), dim3(PRE_BLOCK), 0, st, *P, tiles, tile0, until, seed,
                     chain0, nblk, stride, cnt, qcnt);
  hipLaunchKernelGGL(mpp_prepass_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, (long long)nblk * n_chains, total);
  if (qcnt) hipLaunchKernelGGL(mpp_prepass_scan_kernel, dim3(n_chains), dim3(1024), 0, st, qcnt, (long long)nblk * MPP_NKERNEL, qtot);
  return hipGetLastError();
}
extern "C" hipError_t mpp_prepass_fill(hipStream_t st, const DevParams *P, const TileRef *tiles, int tile0, int n_chains,
                                       const long long *until, unsigned long long seed, unsigned int chain0, int nblk,
                                       long long stride, const unsigned int *off, uint32_t *word, double *rec,
                                       const unsigned int *qcnt, uint32_t *qoff, QEnt *qent, long long *base) {
  hipLaunchKernelGGL(mpp_prepass_fill_kernel, dim3(nblk, n_chains), dim3(PRE_BLOCK), 0, st, *P, tiles, tile0, until, seed,
                     chain0, nblk, stride, off, word, rec, qcnt, qoff, qent, base);
  return hipGetLastError();
}
