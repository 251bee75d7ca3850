// mpp_layout.hpp -- where the arrays of a chain live: each layout written ONCE, as a function that hands its arrays, in memory
// order, to a "walker".  A walker that only adds up bytes gives the size the host asks for, one that hands out pointers
// places the arrays in the kernel: the two cannot drift apart.  Nothing of the kernels is needed here: a stand-alone host
// program can include this header and walk a layout over a host buffer (tests/layout_walk.hip does).
// The form of a pointer walker decides the code the compiler makes of a kernel's prologue, and with it the register
// allocation of the whole kernel (profiles/launch_plumbing.md): LdsCursor, ByteCursor and HbmSlots restate the pointer
// arithmetic the kernels were tuned with.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/mpp_hip.h"

#define STASH 32              // neighbour updates remembered per speculative step
#define CLIP_SLOTS 4          // lanes of one wave that clip at the same time (the others take the next turn)
#define HBM_ALIGN 256
#define DEEP_CLIST 192         // candidate neighbours a wave collects before it evaluates them (>= 64: one cell's entries fit)

struct Rec {                  // one speculative step, fully evaluated
  int kernel, tidx, tslot, has_rem, has_add, valid;
  int ax, ay, rx, ry, pid, ncls;
  int accepted, n_stash, gate_a, _pad;
  int acls, _pad2;            // class of the proposed angle when it is a class edge (KEEP_EDGE_ANGLE), else unused
  double as, ar, aa, aux0, aux1, u_acc, qf, qb, dE;
  double hl, hw, ca, sa, rad, lin_a, ra0, ra1;   // derived data of the proposed point
  double fwd, bwd, log_alpha;                    // filled only when the tile is traced
};

struct Lds {
  double *s, *r, *a, *ca, *sa, *hl, *hw, *rad, *lin, *red0, *red1;
  double *edges;              // [3][32] copy of the mark bin edges
  double *trig;               // [2][32] cos / sin of (angle-class edge + pi/2): the corner trigonometry of a rectangle whose
                              // angle was drawn from the class distribution (data-driven birth / transform) without a sincos
  double *rowbase;            // [H+1] copy of the birth CDF's row level (H <= 1024), else nullptr
  double *stash_v0, *stash_v1;
  double *clip;               // [waves][CLIP_SLOTS][32] polygon buffers of the rectangle clipper
  int *xy;
  unsigned short *order, *cell_items, *cell_cnt, *stash_slot;
  unsigned char *gate;
  Rec *rec;
  int *sh;                    // [0]=n [1]=err [2]=committed ; sh[4..5] = T (double)
};

struct DeepLds {
  uint4 *info;                 // [nmax] (flags | slot, removed xy, added xy, cell coordinates) -- indexed by the step's offset in the round
  uint4 *nb;                   // [nmax] positions (and circumradii, rounded up) of the (at most two) neighbours whose cached
                               // reductions the step changes
  double *st;                  // [nmax][5] ... and their new reductions (2 x 2 values, then the two slots as bits): a step that
                               // commits writes them; only a step that changes more than two neighbours needs a second pass
  uint4 *pw;                   // [nmax] Philox block 0 of the steps, in sorted order (queue rounds: lin_a and gate_a of the
                               // step at that offset, see deep_park)
  unsigned short *poff;        // [nmax] sorted position -> offset of the step in the round
  unsigned short *tcnt;        // [WAVES][16] steps of each kernel type per wave
  double *tring;               // [4 * nmax] temperature of step (offset & mask), filled two rounds ahead
  unsigned long long *racc;    // [WAVES][3][64] per step of a wave: max of the overlaps / min of the alignments with the added point;
                               // a candidate neighbour of the step has a non-finite energy (classic image energies only)
  unsigned int *clist;         // [WAVES][DEEP_CLIST] (step << 16 | slot): the neighbours in range of a wave's steps, in order
  unsigned char *ltab;         // [WAVES][128] the 3 x 3 blocks of cells a wave's steps look at (lane | 0x80: the added point's)
};

// ---- the walkers.  take(f, n): the next array, n elements; same(n, f...): arrays of n elements each, one after the other;
// take_if(f, n): an array that is absent (nullptr) when n == 0; align16(): the next array starts at a multiple of 16 bytes.
// Walkers and layouts are inlined before anything else is optimised (MPP_WALK), and a count keeps the type the layout gives
// it (an int capacity, a size_t product): the compiler then starts from the pointer arithmetic of a hand-written carve.
#define MPP_WALK __host__ __device__ __forceinline__
__host__ __device__ inline size_t hbm_align(size_t b) { return (b + HBM_ALIGN - 1) & ~(size_t)(HBM_ALIGN - 1); }
template <bool HBM = false>   // HBM: every array occupies a multiple of HBM_ALIGN bytes
struct LayoutCount {          // adds up bytes
  size_t bytes = 0;
  MPP_WALK static size_t slot(size_t b) { if constexpr (HBM) return hbm_align(b); else return b; }
  template <class T, class N> MPP_WALK void take(T *&, N n) { bytes += slot((size_t)n * sizeof(T)); }
  template <class T> MPP_WALK void take_if(T *&f, int n) { take(f, n); }
  template <class T, class N, class... U> MPP_WALK void same(N n, T *&, U *&...) { bytes += (1 + sizeof...(U)) * slot((size_t)n * sizeof(T)); }
  MPP_WALK void align16() { bytes = (bytes + 15) & ~(size_t)15; }
};
struct LdsCursor {            // hands out pointers: a typed cursor that moves past each array (the chain's arrays)
  unsigned char *base, *p;
  MPP_WALK explicit LdsCursor(unsigned char *b) : base(b), p(b) {}
  template <class T, class N> MPP_WALK void take(T *&f, N n) { T *q = (T *)p; f = q; p = (unsigned char *)(q + n); }
  template <class T> MPP_WALK void take_if(T *&f, int n) { T *q = (T *)p; f = n > 0 ? q : nullptr; p = (unsigned char *)(q + n); }
  template <class T, class N, class... U> MPP_WALK void same(N n, T *&f, U *&...g) { take(f, n); if constexpr (sizeof...(U) > 0) same(n, g...); }
  MPP_WALK void align16() { size_t off = (size_t)(p - base); off = (off + 15) & ~(size_t)15; p = base + off; }
};
struct ByteCursor {           // hands out pointers: a byte cursor that moves by each array's size (the deep round's arrays)
  unsigned char *p;
  MPP_WALK explicit ByteCursor(unsigned char *b) : p(b) {}
  template <class T> MPP_WALK void take(T *&f, size_t n) { f = (T *)p; p += n * sizeof(T); }
};
struct HbmSlots {             // hands out pointers: base + offset, the k-th of equal arrays at base + k * its slot
  unsigned char *base;
  size_t o = 0;
  MPP_WALK explicit HbmSlots(unsigned char *b) : base(b) {}
  template <class T> MPP_WALK void take(T *&f, size_t n) { f = (T *)(base + o); o += hbm_align(n * sizeof(T)); }
  template <class T, class... U> MPP_WALK void same(size_t n, T *&f, U *&...g) {
    const size_t dc = hbm_align(n * sizeof(T));
    size_t k = 0;
    f = (T *)(base + o);
    ((g = (T *)(base + o + ++k * dc)), ...);
    o += (k + 1) * dc;
  }
};

// ---- the chain in LDS.  mpp_chain_lds_bytes is its count + 64 bytes of slack.
template <class W>
MPP_WALK void chain_layout(W &w, Lds &L, int cap, int ncell, int cell_cap, int spec, int rowbase_n, int waves) {
  w.same(cap, L.s, L.r, L.a, L.ca, L.sa, L.hl, L.hw, L.rad, L.lin, L.red0, L.red1);
  w.take(L.edges, 3 * MPP_NCLASS); w.take(L.trig, 2 * MPP_NCLASS); w.take_if(L.rowbase, rowbase_n);
  w.take(L.stash_v0, (size_t)spec * STASH); w.take(L.stash_v1, (size_t)spec * STASH);
  w.take(L.clip, (size_t)waves * CLIP_SLOTS * 32);
  w.take(L.xy, cap);
  w.take(L.order, cap); w.take(L.cell_items, (size_t)ncell * cell_cap); w.take(L.cell_cnt, ncell);
  w.take(L.stash_slot, (size_t)spec * STASH);
  w.take(L.gate, cap);
  w.align16();
  w.take(L.rec, (size_t)spec); w.take(L.sh, 16);
}
__host__ __device__ inline size_t lds_bytes(int cap, int ncell, int cell_cap, int spec, int rowbase_n, int waves) {
  LayoutCount<> w; Lds L;
  chain_layout(w, L, cap, ncell, cell_cap, spec, rowbase_n, waves);
  return w.bytes + 64;
}
__host__ __device__ inline Lds carve(unsigned char *base, int cap, int ncell, int cell_cap, int spec, int rowbase_n, int waves) {
  LdsCursor w(base); Lds L;
  chain_layout(w, L, cap, ncell, cell_cap, spec, rowbase_n, waves);
  return L;
}

// ---- the HBM-state chain (mpp_sampler_hbm.hip): a chain that outgrows the LDS keeps everything that scales with its
// capacity -- the 11 per-point double arrays, xy, order, gate, cell_items and cell_cnt -- in its own slice of a device
// workspace (hbm_state_layout: each array 256-B aligned); the per-step buffers (edges, trig, rowbase, the stash, clip, rec, sh)
// and the staged parameter block stay in LDS (hbm_lds_layout), whose footprint then no longer depends on the capacity.
template <class W>
MPP_WALK void hbm_state_layout(W &w, Lds &L, int cap, int ncell, int cell_cap) {
  w.same((size_t)cap, L.s, L.r, L.a, L.ca, L.sa, L.hl, L.hw, L.rad, L.lin, L.red0, L.red1);
  w.take(L.xy, (size_t)cap); w.take(L.order, (size_t)cap);
  w.take(L.cell_items, (size_t)ncell * cell_cap); w.take(L.cell_cnt, (size_t)ncell);
  w.take(L.gate, (size_t)cap);
}
template <class W>
MPP_WALK void hbm_lds_layout(W &w, Lds &L, int spec, int rowbase_n, int waves) {
  w.take(L.edges, 3 * MPP_NCLASS); w.take(L.trig, 2 * MPP_NCLASS); w.take_if(L.rowbase, rowbase_n);
  w.take(L.stash_v0, (size_t)spec * STASH); w.take(L.stash_v1, (size_t)spec * STASH);
  w.take(L.clip, (size_t)waves * CLIP_SLOTS * 32);
  w.take(L.stash_slot, (size_t)spec * STASH);
  w.align16();
  w.take(L.rec, (size_t)spec); w.take(L.sh, 16);
}
__host__ __device__ inline size_t hbm_state_bytes(int cap, int ncell, int cell_cap) {
  LayoutCount<true> w; Lds L;
  hbm_state_layout(w, L, cap, ncell, cell_cap);
  return w.bytes;
}
__host__ __device__ inline size_t hbm_lds_bytes(int spec, int rowbase_n, int waves) {
  LayoutCount<> w; Lds L;
  hbm_lds_layout(w, L, spec, rowbase_n, waves);
  return w.bytes + 64;
}
__host__ __device__ inline Lds carve_hbm(unsigned char *lds, unsigned char *ws, int cap, int ncell, int cell_cap, int spec,
                                         int rowbase_n, int waves) {
  HbmSlots s(ws); LdsCursor w(lds); Lds L;
  hbm_state_layout(s, L, cap, ncell, cell_cap);
  hbm_lds_layout(w, L, spec, rowbase_n, waves);
  return L;
}

// ---- the deep rounds (mpp_deep.hip): the chain without stash or step records (spec 0), its end rounded up to 16 bytes,
// then the round's arrays.  mpp_deep_lds_bytes is deep_base_bytes + deep_extra_bytes (the latter with 64 bytes of slack).
template <class W>
MPP_WALK void deep_layout(W &w, DeepLds &D, int nmax, int waves, int ext) {
  w.take(D.pw, (size_t)nmax); w.take(D.tring, (size_t)4 * nmax);
  w.take(D.racc, (size_t)waves * (2 + (ext ? 1 : 0)) * 64); w.take(D.clist, (size_t)waves * DEEP_CLIST);
  w.take(D.info, (size_t)nmax); w.take(D.nb, (size_t)nmax); w.take(D.st, (size_t)nmax * 5);
  w.take(D.poff, (size_t)nmax); w.take(D.tcnt, (size_t)waves * 16); w.take(D.ltab, (size_t)waves * 128);
}
__host__ __device__ inline size_t deep_extra_bytes(int nmax, int waves, int ext) {
  LayoutCount<> w; DeepLds D;
  deep_layout(w, D, nmax, waves, ext);
  return w.bytes + 64;
}
__host__ __device__ inline size_t deep_base_bytes(int cap, int ncell, int cell_cap, int rowbase_n, int waves) {
  return (lds_bytes(cap, ncell, cell_cap, 0, rowbase_n, waves) + 15) & ~(size_t)15;
}
__host__ __device__ inline DeepLds deep_carve(unsigned char *base, int nmax, int waves, int ext) {
  ByteCursor w(base); DeepLds D;
  deep_layout(w, D, nmax, waves, ext);
  return D;
}
