// mpp_hot.hip -- the table form of the hot start: the one-wave-per-step chain of eight waves (mpp_chain_body.inc, the body of
// mpp_chain_kernel) whose steps take their draw from the launch's pre-pass table (mpp_prepass.hpp) instead of computing it.
// A step's kernel type, its accept uniform, the Gaussian kernels' Box-Muller pair and everything of a birth -- the point, the
// marks, the proposal density, the geometry and the unit terms -- depend on the step's Philox words and the score maps alone;
// the pre-pass has them for the deep launch already, with the functions the chain kernels use.  Here a birth loads its
// record and goes straight to the neighbour pass (evaluate_tab_birth), every other step loads its queue entry and finishes
// the proposal against the configuration (draw_tail_q<false>).  Same values, same operations after them: the same chain.
#define MPP_HOT_TABLE 1
// ... and a round's commits go on past an accepted birth or death (DevParams::hot_past; mpp_chain_body.inc, phase B): the
// later records are checked against the new population and order[], and take their accept test again
#define MPP_HOT_PAST 1
#include "mpp_chain.hpp"
#include "mpp_split_merge.hpp"
#include "mpp_launch.hpp"

// The one instantiation the hot start runs: untraced, no split / merge, the specialised pair loops (FAST), two waves per SIMD.
template <int WAVES, int OCC>
__global__ __launch_bounds__(WAVE *WAVES, OCC) void mpp_hot_kernel(const DevParams Pv, const TileRef *tiles, int tile0,
                                                                const long long *until, const PreTab pt) {
  constexpr int LPW = 0;
  constexpr bool DIAG = false, SM = false, FAST = true;
  constexpr long long trace_base = 0;
  constexpr int trace_tile = -1;
  const mpp_proposal *tape = nullptr;
  mpp_step_out *const out = nullptr;
  mpp_proposal *const props = nullptr;
#include "mpp_chain_body.inc"
}

// a.lds: mpp_chain_lds_bytes of the launch (the layout is mpp_chain_kernel's: chain_layout of mpp_layout.hpp); pt: a table with
// queues whose stride is below 2^28 (every step's word then carries its queue position), built for exactly these chains at
// their current steps.  Of the bundle the kernel takes the parameter block, the tile table and the until table.
extern "C" hipError_t mpp_launch_hot(const ChainLaunch &a, const PreTab *pt) {
  if (!pt->word || !pt->qent || pt->stride >= (1ll << 28)) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute((const void *)mpp_hot_kernel<8, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((mpp_hot_kernel<8, 2>), dim3(a.grid), dim3(WAVE * 8), a.lds, a.st, *a.P, a.tiles, a.tile0, a.until, *pt);
  return hipGetLastError();
}
