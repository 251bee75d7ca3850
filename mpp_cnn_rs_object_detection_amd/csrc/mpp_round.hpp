// mpp_round.hpp -- the book of one round of the local descent, and of the completion as its births-only form (k_descent_round,
// mpp_descent.hip; the rule is spelled out at mpp_descend in mpp_hip.h), in plain C++: tests/round_walk.hip walks it on the host.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/mpp_hip.h"
// One round of an open chain: the n_rem values the death half removed and the n_kept values of the candidates the birth half
// kept (k_complete_append has placed them behind the configuration when they fit) are added one after another; a half counts
// only with its bit of `what`.  Births that do not fit are not booked; births that fit leave what mpp_set_points of the longer
// list leaves: *count grows, *err = 0.  Status: 2 the births do not fit, 0 nothing changed, 1 the round limit, else still open.
__host__ __device__ __forceinline__ void descent_book(mpp_descent_report &r, int what, int max_rounds, int cap, int32_t *count,
                                                      int32_t *err, int n_rem, const double *rem_val, int n_kept, const double *gain_val) {
  const int nr = (what & MPP_DESCEND_DEATHS) ? n_rem : 0, nk = (what & MPP_DESCEND_BIRTHS) ? n_kept : 0;
  int n = *count;
  const bool full = nk > 0 && (n < 0 || nk > cap - n);
  const int nb = full ? 0 : nk;                                  // (the births that are booked)
  for (int i = 0; i < nr; ++i) r.gain_deaths += rem_val[i];
  for (int i = 0; i < nb; ++i) r.gain_births += gain_val[i];
  r.n_removed += nr; r.n_added += nb;
  if (nb > 0) { *count = n += nb; *err = 0; }
  const bool changed = nr > 0 || nb > 0;
  r.rounds += changed ? 1 : 0;
  if (full || !changed) r.status = full ? 2 : 0;
  else if (r.rounds >= max_rounds) r.status = 1;
  r.n_after = n < 0 ? 0 : (n > cap ? cap : n);
}
// One round of an open chain of the relocation (k_move_round, mpp_relocate.hip; the rule is spelled out at mpp_relocate in
// mpp_hip.h): the n_kept gains of the points the round rewrote in place are added one after another, in slot order.  The count
// never changes.  Moves leave what mpp_set_points of the edited list leaves: *err = 0.  Status: 0 nothing moved, 1 the round
// limit, else still open.
__host__ __device__ __forceinline__ void relocate_book(mpp_relocate_report &r, int max_rounds, int32_t *err, int n_kept,
                                                       const double *gain_val) {
  for (int i = 0; i < n_kept; ++i) r.gain += gain_val[i];
  r.n_moved += n_kept;
  if (n_kept > 0) *err = 0;
  r.rounds += n_kept > 0 ? 1 : 0;
  if (n_kept <= 0) r.status = 0;
  else if (r.rounds >= max_rounds) r.status = 1;
}
