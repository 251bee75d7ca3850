// mpp_sampler.hip -- the chain kernels (see mpp_chain.hpp for the design notes and the shared pieces)
#include <cstdlib>

#include "mpp_chain.hpp"
#include "mpp_split_merge.hpp"
#include "mpp_launch.hpp"

// WAVES waves per chain.  LPW == 0: one speculative step per wave, the wave's lanes cooperate on it.
// LPW > 0 ("lane mode"): lanes 0..LPW-1 of every wave each evaluate their own step.  SPEC steps per round.
// DIAG = false is the production instantiation: proposals from Philox, nothing recorded (the tape and
// trace code is compiled out, which also lowers the register need of the hot loop).
// OCC: minimum waves per SIMD the register allocation must allow (the hot loop needs ~240 VGPRs: two waves per
// SIMD).  Throughput runs over many one-wave chains ask for OCC = 2 explicitly so that two chains share a SIMD and
// hide each other's latencies.
// SM: the instantiation that also knows the split / merge kernels (mpp_split_merge.hpp); the others carry none of it.
// FAST: the energy model is (pair 0 = rectangle overlap / max, pair 1 = alignment / min) -- both shipped setups; the pair
// loops of eval_delta are then straight-line code (chosen by the host; the generic instantiations cover everything else).
// The body is mpp_chain_body.inc, shared with the HBM-state kernel of mpp_sampler_hbm.hip.
template <int WAVES, int LPW, bool DIAG, int OCC, bool SM, bool FAST = false>
__global__ __launch_bounds__(WAVE *WAVES, OCC) void mpp_chain_kernel(const DevParams Pv, const TileRef *tiles, int tile0,
                                                                  const long long *until, long long trace_base,
                                                                  unsigned long long seed,
                                                                  unsigned int chain0, const mpp_proposal *tape,
                                                                  int trace_tile, mpp_step_out *out,
                                                                  mpp_proposal *props) {
#include "mpp_chain_body.inc"
}

#ifdef MPP_PROFILE
extern "C" __attribute__((visibility("default"))) void mpp_debug_read_prof(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * 16);
}
extern "C" __attribute__((visibility("default"))) void mpp_debug_read_strag(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_strag), sizeof(unsigned long long) * 64);
  unsigned long long z[64] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_strag), z, sizeof z);
}
extern "C" __attribute__((visibility("default"))) void mpp_debug_read_prof4(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof4), sizeof(unsigned long long) * 16);
  unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prof4), z, sizeof z);
}
extern "C" __attribute__((visibility("default"))) void mpp_debug_read_prof3(unsigned long long *out) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof3), sizeof(unsigned long long) * 16);
  unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prof3), z, sizeof z);
}
extern "C" __attribute__((visibility("default"))) void mpp_debug_read_prof2(unsigned long long *out, int reset) {
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof2), sizeof(unsigned long long) * 16);
  (void)hipMemcpyFromSymbol(out + 8, HIP_SYMBOL(g_clip_count), sizeof(unsigned long long));
  if (reset) { unsigned long long z[16] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_prof2), z, sizeof z);
               (void)hipMemcpyToSymbol(HIP_SYMBOL(g_clip_count), z, sizeof(unsigned long long)); }
}
#endif

// until[t] = step[t] + n_steps for the tiles of a launch (set once per host call; re-launches after a capacity overflow
// keep it)
__global__ void k_set_until(const TileRef *tiles, int tile0, int n, long long n_steps, long long *until) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) until[tile0 + i] = *tiles[tile0 + i].step + n_steps;
}
extern "C" void mpp_launch_set_until(hipStream_t st, const TileRef *tiles, int tile0, int n, long long n_steps, long long *until) {
  hipLaunchKernelGGL(k_set_until, dim3((n + 255) / 256), dim3(256), 0, st, tiles, tile0, n, n_steps, until);
}

// ---- host-side launcher ----------------------------------------------------------------------------
extern "C" size_t mpp_chain_lds_bytes(int cap, int ncell, int cell_cap, int spec, int rowbase_n, int waves) {
  return lds_bytes(cap, ncell, cell_cap, spec, rowbase_n, waves);
}
// static LDS a chain kernel with `waves` waves uses besides its dynamic allocation (the staged parameter block of stage_params,
// the same in mpp_chain_kernel, mpp_chain_hbm_kernel, mpp_hot_kernel and mpp_deep_kernel)
extern "C" size_t mpp_chain_static_lds_bytes(int waves) {
  return waves >= MPP_LDS_PARAMS_MIN_WAVES ? ((sizeof(DevParams) + 15) & ~(size_t)15) : 0;
}

template <int WAVES, int LPW, bool DIAG, int OCC, bool SM, bool FAST = false>
static hipError_t launch_spec_d(const ChainLaunch &a) {
  hipError_t e = hipFuncSetAttribute((const void *)mpp_chain_kernel<WAVES, LPW, DIAG, OCC, SM, FAST>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((mpp_chain_kernel<WAVES, LPW, DIAG, OCC, SM, FAST>), dim3(a.grid), dim3(WAVE * WAVES), a.lds, a.st, *a.P, a.tiles,
                     a.tile0, a.until, a.trace_base, a.seed, a.chain0, a.tape, a.trace_tile, a.out, a.props);
  return hipGetLastError();
}
template <int WAVES, int LPW>
static hipError_t launch_spec(const ChainLaunch &a, int occ) {
  constexpr int BASE = (WAVES + 3) / 4;      // waves per SIMD one workgroup needs anyway
  const bool diag = a.tape || a.out || a.props;
  const ModelClass mc = model_class(*a.P);
  if (mc.extended()) {                       // split / merge kernels in the mixture, or a classic image energy: the
                                             // extended instantiations, built for 1 and 8 waves
    if constexpr (LPW == 0 && (WAVES == 1 || WAVES == 8)) {
      if (diag) return launch_spec_d<WAVES, LPW, true, BASE, true>(a);
      return launch_spec_d<WAVES, LPW, false, BASE, true>(a);
    } else {
      return hipErrorNotSupported;
    }
  }
  if (diag) return launch_spec_d<WAVES, LPW, true, BASE, false>(a);
  // the production launches of the shipped energy setups: pair loops specialised (FAST); MPP_NO_FAST=1 keeps the generic code
  if constexpr (LPW == 0 && WAVES <= 8) {
    if (mc.fast && !mc.no_fast) {
      if (WAVES <= 4 && occ >= 2) return launch_spec_d<WAVES, LPW, false, 2, false, true>(a);
      return launch_spec_d<WAVES, LPW, false, BASE, false, true>(a);
    }
  }
  if (WAVES <= 4 && LPW == 0 && occ >= 2) return launch_spec_d<WAVES, LPW, false, 2, false>(a);
  return launch_spec_d<WAVES, LPW, false, BASE, false>(a);
}

// spec = steps evaluated per round; lanes = 0: one wave per step (spec waves); lanes > 0: 4 waves x lanes lanes
extern "C" hipError_t mpp_launch_chain(const ChainLaunch &a, int spec, int lanes, int occ) {
#define GO(W, L) return launch_spec<W, L>(a, occ)
  if (lanes == 0) {
    switch (spec) { case 1: GO(1, 0); case 2: GO(2, 0); case 4: GO(4, 0); case 8: GO(8, 0); case 16: GO(16, 0); }
  } else {
    switch (lanes) { case 1: GO(4, 1); case 2: GO(4, 2); case 4: GO(4, 4); case 8: GO(4, 8); case 16: GO(4, 16); }
  }
#undef GO
  return hipErrorInvalidValue;
}
