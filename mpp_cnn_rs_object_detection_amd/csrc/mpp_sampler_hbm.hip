// mpp_sampler_hbm.hip -- the one-wave-per-step chain with its state in device memory, for the chains that outgrow a
// CU's LDS (see run_chain in mpp_api_chain.hip for the routing, mpp_layout.hpp: hbm_state_layout / hbm_lds_layout for the layout, mpp_chain.hpp: and wave_lds_fence for
// the memory ordering).  Same body as mpp_chain_kernel (mpp_chain_body.inc), same Philox stream, same arithmetic: the
// chain is the one an unlimited LDS would have run.
#define MPP_STATE_HBM 1
#include "mpp_chain.hpp"
#include "mpp_split_merge.hpp"
#include "mpp_launch.hpp"

// WAVES 1 or 8 (one wave per step), generic pair loops (FAST = false); DIAG: traced runs and tape replay; SM: the split /
// merge kernels and the classic image energies.  ws: the workspace, chain blockIdx.x at ws + blockIdx.x * ws_stride.
template <int WAVES, bool DIAG, bool SM>
__global__ __launch_bounds__(WAVE *WAVES, (WAVES + 3) / 4) void mpp_chain_hbm_kernel(
    const DevParams Pv, const TileRef *tiles, int tile0, const long long *until, long long trace_base,
    unsigned long long seed, unsigned int chain0, const mpp_proposal *tape, int trace_tile, mpp_step_out *out,
    mpp_proposal *props, unsigned char *ws, size_t ws_stride) {
  constexpr int LPW = 0;
  constexpr bool FAST = false;
#include "mpp_chain_body.inc"
}

template <int WAVES, bool DIAG, bool SM>
static hipError_t launch_hbm_d(const ChainLaunch &a, unsigned char *ws, size_t ws_stride) {
  hipError_t e = hipFuncSetAttribute((const void *)mpp_chain_hbm_kernel<WAVES, DIAG, SM>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((mpp_chain_hbm_kernel<WAVES, DIAG, SM>), dim3(a.grid), dim3(WAVE * WAVES), a.lds, a.st, *a.P, a.tiles, a.tile0,
                     a.until, a.trace_base, a.seed, a.chain0, a.tape, a.trace_tile, a.out, a.props, ws, ws_stride);
  return hipGetLastError();
}
template <int WAVES>
static hipError_t launch_hbm(const ChainLaunch &a, unsigned char *ws, size_t ws_stride) {
  const bool diag = a.tape || a.out || a.props;
  if (model_class(*a.P).extended())          // split / merge kernels in the mixture, or a classic image energy
    return diag ? launch_hbm_d<WAVES, true, true>(a, ws, ws_stride) : launch_hbm_d<WAVES, false, true>(a, ws, ws_stride);
  return diag ? launch_hbm_d<WAVES, true, false>(a, ws, ws_stride) : launch_hbm_d<WAVES, false, false>(a, ws, ws_stride);
}

// bytes of one chain's workspace slice (a multiple of 256) and of the kernel's dynamic LDS
extern "C" size_t mpp_chain_hbm_state_bytes(int cap, int ncell, int cell_cap) { return hbm_state_bytes(cap, ncell, cell_cap); }
extern "C" size_t mpp_chain_hbm_lds_bytes(int spec, int rowbase_n) { return hbm_lds_bytes(spec, rowbase_n, spec); }

// waves: 1 (contexts with spec_waves 1) or 8 (every other context: speculation does not change the chain)
extern "C" hipError_t mpp_launch_chain_hbm(const ChainLaunch &a, int waves, unsigned char *ws, size_t ws_stride) {
  if (waves == 1) return launch_hbm<1>(a, ws, ws_stride);
  if (waves == 8) return launch_hbm<8>(a, ws, ws_stride);
  return hipErrorInvalidValue;
}
