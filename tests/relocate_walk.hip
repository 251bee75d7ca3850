// relocate_walk.hip -- the book of one relocation round (relocate_book, csrc/mpp_round.hpp) walked on the host against a plain
// restatement of the rule of mpp_relocate (include/mpp_hip.h): random sequences of rounds, every field compared after every
// round, the doubles by their bits.  Built for the host with the address and undefined-behaviour sanitizers by
// tests/test_relocate_book_host.py; prints counters as name=value.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mpp_cnn_rs_object_detection_amd/csrc/mpp_round.hpp"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 32);
}
// +-m 2^e: sums whose bits show the order of the additions
static double value() {
  const double m = (double)(1 + rnd() % 1000), s = (rnd() & 1) ? -1.0 : 1.0;
  int e = (int)(rnd() % 80) - 40;
  double v = s * m;
  for (; e > 0; --e) v *= 2.0;
  for (; e < 0; ++e) v *= 0.5;
  return v;
}
static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, sizeof b); return b; }

// the rule as mpp_hip.h words it, one round of an open chain
struct Plain { int status, rounds, n_moved; double gain; int err; };
static void plain_round(Plain &p, int max_rounds, const std::vector<double> &kept) {
  double g = p.gain;
  for (size_t i = 0; i < kept.size(); ++i) g = g + kept[i];
  p.gain = g;
  p.n_moved += (int)kept.size();
  if (kept.empty()) { p.status = 0; return; }
  p.err = 0;
  p.rounds += 1;
  if (p.rounds >= max_rounds) p.status = 1;
}

int main() {
  long sequences = 0, mismatches = 0, still_open = 0, end0 = 0, end1 = 0, from_error = 0, several = 0, untouched_mismatches = 0;
  for (int seq = 0; seq < 60000; ++seq) {
    const int cap = 1 + (int)(rnd() % 16), max_rounds = 1 + (int)(rnd() % 6), n = (int)(rnd() % (cap + 1));
    int32_t err = (rnd() % 4 == 0) ? 1 + (int32_t)(rnd() % 4) : 0;
    if (err) ++from_error;
    mpp_relocate_report r{};
    r.status = -1; r.n_after = n; r.slot_max = -1; r.max_gain = -1.0;
    Plain p{-1, 0, 0, 0.0, err};
    int round = 0;
    bool two = false;
    for (; round <= max_rounds && r.status < 0; ++round) {
      // (the exact size: a read past the round's list is the sanitizer's to find)
      const int k = (n > 0 && rnd() % 5 != 0) ? 1 + (int)(rnd() % n) : 0;
      std::vector<double> kept(k);
      for (int i = 0; i < k; ++i) kept[i] = value();
      two = two || k >= 2;
      relocate_book(r, max_rounds, &err, k, kept.data());
      plain_round(p, max_rounds, kept);
      if (r.status != p.status || r.rounds != p.rounds || r.n_moved != p.n_moved || bits(r.gain) != bits(p.gain) || err != p.err)
        ++mismatches;
      // the fields the book does not own
      if (r.n_after != n || r.slot_max != -1 || r.n_positive != 0 || bits(r.max_gain) != bits(-1.0)) ++untouched_mismatches;
    }
    if (r.status < 0) ++still_open;
    end0 += r.status == 0; end1 += r.status == 1;
    several += two && r.rounds >= 2;
    ++sequences;
  }
  printf("sequences=%ld mismatches=%ld untouched_mismatches=%ld still_open=%ld end0=%ld end1=%ld from_error=%ld several=%ld\n",
         sequences, mismatches, untouched_mismatches, still_open, end0, end1, from_error, several);
  return mismatches || untouched_mismatches || still_open ? 1 : 0;
}
