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
// step when the table is built (PreTab::base; the pre-pass runs on the stream before the first launch that reads it):
//   word[chain * stride + s - step0] = kernel type (bits 0..3) | birth ordinal << 4 (births); with the queues and
//                                      stride < 2^28, every other step: | its position p in qent << 4 (the hot start reads it)
// and per birth (ordinal, over all chains of the launch) PRE_REC_DOUBLES values, six 16-byte pairs:
//   (u_acc, qf) (as, ar) (aa, lin_a) (hl, hw) (ca, sa) (rad, bits: ax | ay << 16 | (gate_a) << 32)
// (qb of a birth is always 1: proposal_densities() sets it so for both births)
//
// With the queues (option prepass_queues, 8 waves, mpp_deep.hip's QUE instantiation) the pre-pass also sorts every chain's
// steps by kernel type, in step order within a type -- one queue per type -- so that a deep round finds its steps without
// computing a single type:
//   qcnt[(chain * MPP_NKERNEL + t) * nblk + b]  (scanned, per chain) the queue position of the first type-t step of block b:
//                                               qcnt[(chain * MPP_NKERNEL + t) * nblk] is where queue t starts, qtot[chain]
//                                               where the last one ends
//   qoff[chain * stride + p]                    the step (s - step0) at queue position p
//   qent[chain * stride + p]                    what of that step does not depend on the configuration (QEnt)
struct QEnt {
  uint32_t off;                // s - step0
  uint32_t w2;                 // Philox word 2 (the target: mulhi32(w2, n)); a birth: its ordinal in `rec`
  double u_acc;                // the accept test's uniform (births: in their record)
  double a, b;                 // the kernel's own draw: Gaussian translation sigma * (z0, z1); data-driven translation
                               // u53(w3, w4); Gaussian transform the mark offset and pid; data-driven transform u32d(w4) and pid
};
struct PreTab {
  const uint32_t *word;
  const double *rec;
  long long stride;
  const uint32_t *qoff;        // nullptr: no queues
  const QEnt *qent;
  const unsigned int *qcnt;
  const unsigned long long *qtot;
  int qnblk;
  const long long *base;       // per chain of the launch: the step its part of the table starts at (nullptr: the chain's step when
                               // the launch starts).  A launch that finds its chain beyond it starts in mid-table: the hot start's
                               // re-launch after a capacity stop, the deep launch after the handover
};
#define PRE_REC_DOUBLES 12
#define PRE_REC_BYTES (PRE_REC_DOUBLES * 8)
#define PRE_BLOCK 256            // steps per block of the pre-pass kernels
