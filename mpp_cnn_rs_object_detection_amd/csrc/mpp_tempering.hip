// mpp_tempering.hip -- the exchange step of parallel tempering (replica exchange; DESIGN.md section 14, include/mpp_hip.h:
// mpp_run_tempered).  The R replicas of a tile anneal by schedules that differ by a factor per rung of a temperature ladder;
// at an exchange two chains on neighbouring rungs swap their schedules with the Metropolis test of the pair's joint
// Boltzmann weight.  The chain kernels read a chain's schedule from its triple in device memory and write the current
// temperature back, so the swap of two triples is all an exchange has to do: no chain kernel knows of it.
#include <cmath>

#include "mpp_launch.hpp"

// One thread per (tile i, attempted pair j) of exchange e at absolute step s.  The pairs of an exchange are disjoint, so a
// thread is the only one that writes the triples, the rungs and the counter it touches, and the only one that reads them
// for a decision: no atomics.  A thread looks for the two chains of its rungs among the tile's R replicas; the rungs that
// the tile's other pairs swap meanwhile are never k or k + 1, whichever of their two values it sees.
__global__ void k_exchange(const TileRef *tiles, int n_maps, int R, int n_pairs, int k0, double *sched, int32_t *rung,
                           const double *energy, long long s, unsigned long long seed, unsigned int chain0, long long *accepted,
                           mpp_exchange_record *log, long long log_base, long long log_cap) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_maps * n_pairs) return;
  const int i = g / n_pairs, k = k0 + 2 * (g - i * n_pairs);
  int a = -1, b = -1;
  for (int r = 0; r < R; ++r) {
    const int t = r * n_maps + i, v = rung[t];
    if (v == k) a = t;
    else if (v == k + 1) b = t;
  }
  if (a < 0 || b < 0) return;                          // (a ladder is a permutation per tile: both are found)
  const double Ea = energy[a], Eb = energy[b];
  double *sa = sched + 3 * (size_t)a, *sb = sched + 3 * (size_t)b;
  const double Ta = sa[0], Tb = sb[0];
  const double d = (1.0 / Ta - 1.0 / Tb) * (Ea - Eb);
  // the key of replica 0 of the tile: entry i of the table (mpp_set_chain_keys in force: its own, else the launch's)
  const TileRef &t0 = tiles[i];
  const unsigned long long key = t0.key_on ? (unsigned long long)t0.key_seed : seed;
  const uint32_t chain = t0.key_on ? t0.key_chain : chain0 + (uint32_t)i;
  uint32_t w[4];
  philox4x32_10((uint32_t)s, (uint32_t)((unsigned long long)s >> 32), 0x80000000u | (uint32_t)k, chain, (uint32_t)key,
                (uint32_t)(key >> 32), w);
  const double u = u53(w[0], w[1]);
  const bool acc = Ta > 0.0 && Tb > 0.0 && isfinite(Ea) && isfinite(Eb) && (d >= 0.0 || u < exp(d));
  if (acc) {
    for (int j = 0; j < 3; ++j) { const double v = sa[j]; sa[j] = sb[j]; sb[j] = v; }
    rung[a] = k + 1; rung[b] = k;
    accepted[(size_t)i * (R - 1) + k] += 1;
  }
  const long long at = log_base + g;
  if (log && at < log_cap) {
    mpp_exchange_record rec;
    rec.step = s; rec.tile = i; rec.k = k; rec.chain_a = a; rec.chain_b = b; rec.accepted = acc ? 1 : 0; rec._pad = 0;
    rec.Ea = Ea; rec.Eb = Eb; rec.Ta = Ta; rec.Tb = Tb; rec.u = u;
    log[at] = rec;
  }
}

// pairs (k, k + 1), k + 1 < R: R = 2 has one and attempts it at every exchange; R > 2 attempts those with k % 2 == e % 2
extern "C" void mpp_launch_exchange(hipStream_t st, const TileRef *tiles, int n_maps, int R, double *sched, int32_t *rung,
                                    const double *energy, long long s, long long e, unsigned long long seed, unsigned int chain0,
                                    long long *accepted, mpp_exchange_record *log, long long log_base, long long log_cap) {
  const int k0 = R == 2 ? 0 : (int)(e & 1), n_pairs = (R - k0) / 2;
  const long long n = (long long)n_maps * n_pairs;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_exchange, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, tiles, n_maps, R, n_pairs, k0, sched, rung, energy,
                     s, seed, chain0, accepted, log, log_base, log_cap);
}
