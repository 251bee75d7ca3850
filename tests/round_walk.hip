// round_walk.hip -- host program of tests/test_round_rule_host.py: the book of a round of the local descent
// (csrc/mpp_round.hpp, descent_book, the function k_descent_round calls) against the two kernels it replaced, on random
// sequences of rounds.  Every sequence is walked twice from one start: through descent_book with the chain's one record, and
// through a transcription of the former pair -- k_complete_round, which booked the births into a second record per chain (an
// mpp_complete_report, launched with a round limit of 1 << 30 that never bound) and moved the count, followed by
// k_descent_round, which copied n_added and the gain out of that record, applied max_rounds and wrote its status back into it.
// What lies outside the book is shared by both walks: the death half's compaction takes n_rem points off the count (and zeroes
// the error word) before the book, as k_descent_remove does.  After every round every field of the descent report (doubles by
// their bits), the count and the error word must be equal; with what = births the record mpp_birth_complete now fills from the
// descent report must be the second record of the transcription.  (Its n_after was the raw count, the descent's is the count
// within 0 .. cap: they differ only from the error state, a negative count, which no call of the library leaves; there the
// field is not compared.)  Built for the host only, with -fsanitize=address,undefined.  Prints the number of sequences, of
// mismatches, and what the sequences held; the exit status is 1 when a round differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../mpp_cnn_rs_object_detection_amd/csrc/mpp_round.hpp"

enum { CAP_MAX = 16 };

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {                                          // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }   // 0 .. n-1
static double value() {                                          // +-m * 2^e, e in -20 .. 20: the order of the additions shows
  const double m = (double)(1 + below(1 << 20));
  return std::ldexp(below(2) ? m : -m, below(41) - 20);
}

// ---- the transcription of the two kernels (one chain; n: the chain's count, err: its error word)
static int count_in(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

static void old_complete_round(int32_t *tn, int32_t *terr, int cap, int k, const double *gain_val, int max_rounds, mpp_complete_report *rep) {
  mpp_complete_report r = *rep;
  if (r.status >= 0) return;
  int n = *tn;
  if (k == 0) r.status = 0;
  else if (n < 0 || k > cap - n) r.status = 2;
  else {
    double g = r.gain;
    for (int i = 0; i < k; ++i) g += gain_val[i];
    r.gain = g;
    n += k;
    *tn = n; *terr = 0;
    r.rounds += 1; r.n_added += k;
    if (r.rounds >= max_rounds) r.status = 1;
  }
  r.n_after = n;
  *rep = r;
}

static void old_descent_round(const int32_t *tn, int cap, int what, int max_rounds, int n_rem, const double *rem_val,
                              mpp_descent_report *rep, mpp_complete_report *crep) {
  mpp_descent_report r = *rep;
  if (r.status >= 0) return;
  bool changed = false, full = false;
  if (what & MPP_DESCEND_DEATHS) {
    const int k = n_rem;
    if (k > 0) {
      double g = r.gain_deaths;
      for (int i = 0; i < k; ++i) g += rem_val[i];
      r.gain_deaths = g;
      r.n_removed += k;
      changed = true;
    }
  }
  if (what & MPP_DESCEND_BIRTHS) {
    const mpp_complete_report b = *crep;
    full = b.status == 2;
    if (b.n_added > r.n_added) { r.n_added = b.n_added; r.gain_births = b.gain; changed = true; }
  }
  if (changed) r.rounds += 1;
  if (full) r.status = 2;
  else if (!changed) r.status = 0;
  else if (r.rounds >= max_rounds) r.status = 1;
  r.n_after = count_in(*tn, cap);
  *rep = r;
  crep->status = r.status;
}

// ---- what k_descent_init (and the former k_complete_init) leave
static mpp_descent_report open_report(int n) {
  mpp_descent_report r;
  std::memset(&r, 0, sizeof r);
  r.status = -1; r.n_after = n; r.slot_max = -1; r.max_p = -HUGE_VAL; r.x = -1; r.y = -1;
  return r;
}
static mpp_complete_report open_complete() {
  mpp_complete_report r;
  std::memset(&r, 0, sizeof r);
  r.status = -1; r.x = -1; r.y = -1;
  return r;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
  const long long sequences = 200000;
  long long mismatches = 0, complete_mismatches = 0, still_open = 0, rounds_walked = 0, end[3] = {0, 0, 0};
  long long both_halves = 0, full_after_deaths = 0, births_two_rounds = 0, from_error = 0;
  for (long long q = 0; q < sequences; ++q) {
    const int cap = 1 + below(CAP_MAX), max_rounds = 1 + below(6), what = 1 + below(3);
    const bool error_state = below(8) == 0;
    const int start = error_state ? -1 : below(cap + 1);
    from_error += error_state;
    int32_t n_new = start, n_old = start, err_new = 7, err_old = 7;
    mpp_descent_report r_new = open_report(count_in(start, cap)), r_old = r_new;
    mpp_complete_report c_old = open_complete();
    int birth_rounds = 0;
    for (int round = 0; round <= max_rounds && r_old.status < 0; ++round) {
      double rem_val[CAP_MAX], gain_val[CAP_MAX];
      for (int i = 0; i < CAP_MAX; ++i) { rem_val[i] = value(); gain_val[i] = value(); }
      // the death half: n_rem of the chain's points leave (drawn without deaths too: the book has to ignore it)
      const int have = count_in(n_old, cap), n_rem = below(3) == 0 ? 0 : below(have + 1);
      if ((what & MPP_DESCEND_DEATHS) && n_rem > 0) { n_old = n_new = have - n_rem; err_old = err_new = 0; }
      // the birth half: n_kept candidates; a third of the draws fit for sure, a quarter are none
      const int room = cap - count_in(n_old, cap), pick = below(4);
      const int n_kept = pick == 0 ? 0 : (pick == 1 ? 1 + below(cap) : below(room + 1));
      const int removed_before = r_old.n_removed, added_before = r_old.n_added;

      if (what & MPP_DESCEND_BIRTHS) old_complete_round(&n_old, &err_old, cap, n_kept, gain_val, 1 << 30, &c_old);
      old_descent_round(&n_old, cap, what, max_rounds, n_rem, rem_val, &r_old, &c_old);
      descent_book(r_new, what, max_rounds, cap, &n_new, &err_new, n_rem, rem_val, n_kept, gain_val);
      ++rounds_walked;

      const bool equal = r_new.status == r_old.status && r_new.rounds == r_old.rounds && r_new.n_added == r_old.n_added &&
                         r_new.n_removed == r_old.n_removed && r_new.n_after == r_old.n_after && r_new.slot_max == r_old.slot_max &&
                         same_bits(r_new.gain_births, r_old.gain_births) && same_bits(r_new.gain_deaths, r_old.gain_deaths) &&
                         same_bits(r_new.max_p, r_old.max_p) && same_bits(r_new.min_dE, r_old.min_dE) && r_new.x == r_old.x &&
                         r_new.y == r_old.y && r_new.n_positive == r_old.n_positive && r_new.n_negative == r_old.n_negative &&
                         r_new.n_nan == r_old.n_nan && n_new == n_old && err_new == err_old;
      if (!equal) {
        if (mismatches < 5)
          std::fprintf(stderr, "sequence %lld round %d (cap %d, max_rounds %d, what %d, start %d, n_rem %d, n_kept %d): status %d / %d, "
                       "rounds %d / %d, count %d / %d, gains %a %a / %a %a\n", q, round, cap, max_rounds, what, start, n_rem, n_kept,
                       r_new.status, r_old.status, r_new.rounds, r_old.rounds, n_new, n_old, r_new.gain_births, r_new.gain_deaths,
                       r_old.gain_births, r_old.gain_deaths);
        ++mismatches;
      }
      if (what == MPP_DESCEND_BIRTHS) {                          // the record mpp_birth_complete fills on the host
        const bool same = r_new.status == c_old.status && r_new.rounds == c_old.rounds && r_new.n_added == c_old.n_added &&
                          same_bits(r_new.gain_births, c_old.gain) && (error_state || r_new.n_after == c_old.n_after);
        complete_mismatches += same ? 0 : 1;
      }
      const bool died = r_old.n_removed > removed_before, born = r_old.n_added > added_before;
      both_halves += died && born;
      full_after_deaths += r_old.status == 2 && died && !born;
      birth_rounds += born;
    }
    if (r_old.status < 0 || r_new.status < 0) ++still_open;
    else end[r_old.status] += 1;
    births_two_rounds += birth_rounds >= 2;
  }
  std::printf("sequences=%lld rounds=%lld mismatches=%lld complete_mismatches=%lld still_open=%lld end0=%lld end1=%lld end2=%lld "
              "both_halves=%lld full_after_deaths=%lld births_two_rounds=%lld from_error=%lld\n", sequences, rounds_walked, mismatches,
              complete_mismatches, still_open, end[0], end[1], end[2], both_halves, full_after_deaths, births_two_rounds, from_error);
  return mismatches || complete_mismatches || still_open ? 1 : 0;
}
