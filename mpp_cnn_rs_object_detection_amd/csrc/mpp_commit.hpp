// mpp_commit.hpp -- the step reports of a deep round (mpp_deep.hip) and the test the commit decision is made of: does a
// committed move / transform q make a later report o untrustworthy?  Nothing of the kernels is needed here: a stand-alone
// host program can include this header and decide windows of reports on the CPU (tests/commit_walk.hip does).
//
// The decision is a function of the round's reports alone, and it needs no order ("The deep-round kernel", 5.):
//   S  the first report that is invalid, or that some changing report before it conflicts with (commit_conflict);
//   T  the first changing report that ends the round: its cell is full (DI_FULL), or it is a birth / death;
//   T < S: step T decides (cell overflow: the round commits T steps; a death, a birth: T + 1; a birth at capacity: point
//          overflow, T steps); otherwise the round commits S steps (and reports a bad target if report S has DI_BAD).
// Only changing reports below min(T, first invalid report) can move S below it: the others are not tested.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>

// info word 0: bits 0..15 slot, then flags
#define DI_VALID (1 << 16)
#define DI_CHG (1 << 17)
#define DI_HR (1 << 18)
#define DI_HA (1 << 19)
#define DI_BAD (1 << 20)     // the proposal could not be formed (reported when the commit reaches it)
#define DI_ACC (1 << 21)
#define DI_FULL (1 << 22)    // the cell the step adds to is full (capacity check, made against the round's start state)
#define DI_NB (1 << 23)      // the step changes cached reductions of neighbours: committing it needs the second pass
#define DI_NBOV (1 << 24)    // ... of more than two neighbours (their positions are not all reported)
#define DI_NB2 (1 << 26)     // ... of at least two neighbours
#define DI_RESC (1 << 25)    // the evaluation re-reduced a neighbour: it looked two interaction ranges away
#define DI_KEPT (1 << 27)    // (queue rounds, option deep_carry) the report outlived the round it was made in: see carry_keeps

// a changing report that ends the round when the commit reaches it
__host__ __device__ __forceinline__ bool commit_terminal(unsigned f) {
  return (f & DI_CHG) && ((f & DI_FULL) || !((f & DI_HR) && (f & DI_HA)));
}

// Is the later report o still trustworthy after the move / transform q commits?  Not when o read something q writes:
// the slot itself; a rectangle within the interaction range of o's points, before or after (q's slot); a neighbour whose
// cached reductions q changes and o used (q reports up to two of them; more: twice the range); a cell list of o's 3 x 3
// blocks (q crosses a cell border: the order of that cell's entries changes); and, when o re-reduced a neighbour, anything
// within twice the range.
// q, o: the reports (D.info); qn: q's neighbour word (D.nb: two positions, their radii, q's own reach in .w); o_r: o's reach;
// range2: the longest interaction range, far2: the conflict range of a step that looked further, align2: the alignment
// term's range (all squared).
__host__ __device__ __forceinline__ bool commit_conflict(const uint4 &q, const uint4 &qn, const uint4 &o, int o_r, int range2,
                                                         int far2, int align2) {
  const int qf = (int)q.x;
  const int q_ts = qf & 0xffff;
  const int qx[2] = {(int)(q.y & 0xffffu), (int)(q.z & 0xffffu)}, qy[2] = {(int)(q.y >> 16), (int)(q.z >> 16)};
  const int qci[2] = {(int)(q.w & 0xffu), (int)((q.w >> 16) & 0xffu)}, qcj[2] = {(int)((q.w >> 8) & 0xffu), (int)(q.w >> 24)};
  const bool q_cross = qci[0] != qci[1] || qcj[0] != qcj[1];
  const bool q_far = (qf & DI_NBOV) != 0;
  int qnx[2] = {0, 0}, qny[2] = {0, 0}, qnr[2] = {0, 0}, q_nnb = 0;
  const int q_r = (int)qn.w;
  if (qf & DI_NB) {
    qnx[0] = (int)(qn.x & 0xffffu); qny[0] = (int)(qn.x >> 16); qnx[1] = (int)(qn.y & 0xffffu); qny[1] = (int)(qn.y >> 16);
    qnr[0] = (int)(qn.z & 0xffu); qnr[1] = (int)((qn.z >> 8) & 0xffu);
    q_nnb = 1;
  }
  const bool q_nb2 = (qf & DI_NB2) != 0;
  const int of = (int)o.x;
  const bool oh[2] = {(of & DI_HR) != 0, (of & DI_HA) != 0};
  const int ox[2] = {(int)(o.y & 0xffffu), (int)(o.z & 0xffffu)}, oy[2] = {(int)(o.y >> 16), (int)(o.z >> 16)};
  const int oci[2] = {(int)(o.w & 0xffu), (int)((o.w >> 16) & 0xffu)}, ocj[2] = {(int)((o.w >> 8) & 0xffu), (int)(o.w >> 24)};
  // how far two rectangles can see each other: the alignment term its range, the overlap term as far as the
  // circumscribed circles meet (radii rounded up, + 1 px for the rounding and the 1e-7 of the circle test), neither
  // beyond the terms' cut-off
  auto reach2 = [&](int ra, int rb) { const int t = (ra + rb + 1) * (ra + rb + 1), a2 = align2; const int m = t > a2 ? t : a2; return m < range2 ? m : range2; };
  const int lim2 = ((of & (DI_RESC | DI_NBOV)) || q_far) ? far2 : reach2(o_r, q_r);
  bool bad = oh[0] && (of & 0xffff) == q_ts;
#pragma unroll
  for (int a = 0; a < 2; ++a)
    if (oh[a]) {
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int dx = ox[a] - qx[b], dy = oy[a] - qy[b];
        if (dx * dx + dy * dy <= lim2) bad = true;
        if (q_cross && abs(oci[a] - qci[b]) <= 1 && abs(ocj[a] - qcj[b]) <= 1) bad = true;
      }
      if (q_nnb > 0) {
        const int dx0 = ox[a] - qnx[0], dy0 = oy[a] - qny[0];
        if (dx0 * dx0 + dy0 * dy0 <= reach2(o_r, qnr[0])) bad = true;
        const int dx1 = ox[a] - qnx[1], dy1 = oy[a] - qny[1];
        if (q_nb2 && dx1 * dx1 + dy1 * dy1 <= reach2(o_r, qnr[1])) bad = true;
      }
    }
  return bad;
}

// Kept reports (option deep_carry).  A round ends at the first report a committed change makes untrustworthy; the reports
// behind it are evaluated against the very state the next round starts from, unless a change that committed wrote something
// they read.  Report o of the window, at offset idx, stays trustworthy for the next round iff
//   it is valid and does not change the state (a changing step is evaluated again: deep_mutate wants its record);
//   it lies at or behind the committed count, and is not the report S at which the round ended;
//   the round committed no birth or death (n and order[] are what o was evaluated against);
//   commit_conflict(q, qn, o, ...) is false for EVERY changing report q that committed in this round.
// The last condition arrives as first_q: the lowest offset of a changing report below min(T, first invalid report) that
// conflicts with o (CARRY_NO_Q: none).  Those are the reports the commit decision tests anyway; every changing report that
// commits without ending the round is among them, and one of them committed iff its offset is below the committed count.
// No order is needed here either: first_q is a minimum over pair tests that do not depend on each other.
#define CARRY_NO_Q 0xffffffffu
__host__ __device__ __forceinline__ bool carry_keeps(unsigned of, int idx, int committed, int s_end, bool pop_changed, unsigned first_q) {
  return (of & DI_VALID) && !(of & DI_CHG) && idx >= committed && idx != s_end && !pop_changed && first_q >= (unsigned)committed;
}
