// mpp_prepass.hpp -- the table of a deep launch's births, computed before the chain by a wide kernel (mpp_prepass.hip).
//
// A birth (uniform or data-driven) draws its point, marks, proposal density and accept uniform from the step's Philox
// words and the score maps alone, and its geometry and unit terms are functions of those: nothing of it depends on the
// configuration.  In a deep round the data-driven birth was the slowest lane of the slowest wave (the two-level CDF
// search, then three mark rows one after the other).  The pre-pass does that work for every step of the launch on the
// otherwise idle CUs; the deep kernel's birth lanes load the result.
#pragma once
#include <cstdint>

// per chain of the launch (launch-local index, the deep kernel's blockIdx.x) and step s in [step0, until), step0 the chain's
// step when the launch starts (the pre-pass runs on the launch's stream right before it):
//   word[chain * stride + s - step0] = kernel type (bits 0..3) | birth ordinal << 4 (births only)
// and per birth (ordinal, over all chains of the launch) PRE_REC_DOUBLES values, six 16-byte pairs:
//   (u_acc, qf) (as, ar) (aa, lin_a) (hl, hw) (ca, sa) (rad, bits: ax | ay << 16 | (gate_a) << 32)
// (qb of a birth is always 1: proposal_densities() sets it so for both births)
struct PreTab {
  const uint32_t *word;
  const double *rec;
  long long stride;
};
#define PRE_REC_DOUBLES 12
#define PRE_REC_BYTES (PRE_REC_DOUBLES * 8)
#define PRE_BLOCK 256            // steps per block of the pre-pass kernels
