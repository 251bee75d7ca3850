// commit_walk.hip -- host program of tests/test_commit_rule_host.py: the commit decision of a deep round (csrc/mpp_deep.hip,
// phase C) on random windows of step reports, twice: as the serial loop the kernel ran before the decision was dealt to
// the waves (a literal transcription: one iteration per committed changing step, each updating which later reports are
// still trustworthy), and in the order-free form of csrc/mpp_commit.hpp as the kernel has it now (eight waves, the relevant
// changing steps dealt round-robin, the waves' first conflicts combined by minimum).  Both use the pair test of the
// header.  Built for the host only, with -fsanitize=address,undefined.  Prints the number of windows, of mismatches, and
// of windows by the way their round ends; the exit status is 1 when a window differs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mpp_cnn_rs_object_detection_amd/csrc/mpp_commit.hpp"

enum { ERR_NONE = 0, ERR_POINT = 1, ERR_CELL = 2, ERR_BAD = 3 };     // (which error, not the library's codes)
enum { WAVES = 8, NCH = 4 };

struct Window {
  int lim, n, cap, range2, far2, align2;
  std::vector<uint4> info, nb;
};
struct Outcome {
  int committed, err, cur_n;
  unsigned long long mask[NCH];
  bool any_commit, any_apply;
  bool operator==(const Outcome &o) const {
    for (int i = 0; i < NCH; ++i) if (mask[i] != o.mask[i]) return false;
    return committed == o.committed && err == o.err && cur_n == o.cur_n && any_commit == o.any_commit && any_apply == o.any_apply;
  }
};

static unsigned long long low_mask(int k) { return k <= 0 ? 0ull : (k >= 64 ? ~0ull : ((1ull << k) - 1ull)); }
static int first_bit(unsigned long long m) { return __builtin_ctzll(m); }

// ---- the serial loop
static Outcome decide_serial(const Window &w) {
  const int lim = w.lim;
  std::vector<char> ok(lim);
  for (int i = 0; i < lim; ++i) ok[i] = (w.info[i].x & DI_VALID) != 0;
  Outcome r{};
  int cur = 0, err = ERR_NONE, committed = 0, cur_n = w.n;
  bool any_commit = false, any_apply = false;
  while (true) {
    int first_bad = lim;
    for (int i = lim - 1; i >= 0; --i) if (!ok[i]) first_bad = i;
    int wq = -1;
    for (int i = first_bad - 1; i >= cur; --i) if (w.info[i].x & DI_CHG) wq = i;
    if (wq < 0) {
      committed = first_bad;
      if (first_bad < lim && (w.info[first_bad].x & DI_BAD)) err = ERR_BAD;
      break;
    }
    const uint4 q = w.info[wq];
    const int qf = (int)q.x;
    const bool q_hr = qf & DI_HR, q_ha = qf & DI_HA;
    if (qf & DI_FULL) { err = ERR_CELL; committed = wq; break; }
    if (!(q_hr && q_ha)) {
      if (q_hr) cur_n -= 1;
      else if (cur_n >= w.cap) { err = ERR_POINT; committed = wq; break; }
      else cur_n += 1;
      r.mask[wq >> 6] |= 1ull << (wq & 63);
      any_commit = true;
      if (qf & DI_NBOV) any_apply = true;
      committed = wq + 1;
      break;
    }
    r.mask[wq >> 6] |= 1ull << (wq & 63);
    any_commit = true;
    if (qf & DI_NBOV) any_apply = true;
    const uint4 qn = w.nb[wq];
    for (int idx = wq + 1; idx < lim; ++idx)
      if (ok[idx] && commit_conflict(q, qn, w.info[idx], (int)w.nb[idx].w, w.range2, w.far2, w.align2)) ok[idx] = false;
    cur = wq + 1;
  }
  r.committed = committed; r.err = err; r.cur_n = cur_n; r.any_commit = any_commit; r.any_apply = any_apply;
  return r;
}

// ---- the order-free form, as phase C has it; how[0]: 0 no end within the window, 1 a conflict, 2 an invalid report, 3 step T
static Outcome decide_split(const Window &w, int *how) {
  const int lim = w.lim, nch = (lim + 63) >> 6;
  unsigned long long am[NCH] = {0, 0, 0, 0};
  int first_inv = lim, t_end = lim;
  for (int i = lim - 1; i >= 0; --i) {
    const unsigned f = w.info[i].x;
    if (f & DI_CHG) am[i >> 6] |= 1ull << (i & 63);
    if (!(f & DI_VALID)) first_inv = i;
    if (commit_terminal(f)) t_end = i;
  }
  const int bound = t_end < first_inv ? t_end : first_inv;
  int nrel = 0;
  for (int ch = 0; ch < NCH; ++ch) nrel += __builtin_popcountll(am[ch] & low_mask(bound - ch * 64));
  int s_wave[WAVES];
  for (int wv = 0; wv < WAVES; ++wv) {
    int s_end = first_inv, cur = 0;
    const bool deal = nrel > 1;
    for (int k = 0; k < nrel; ++k) {
      int wq = -1;
      for (int ch = NCH - 1; ch >= 0; --ch) {
        const unsigned long long t = am[ch] & ~low_mask(cur - ch * 64) & low_mask(bound - ch * 64);
        if (t) wq = ch * 64 + first_bit(t);
      }
      cur = wq + 1;
      if (deal && (k & (WAVES - 1)) != wv) continue;
      const uint4 q = w.info[wq], qn = w.nb[wq];
      for (int ch = 0; ch < NCH; ++ch)
        if (ch < nch && ch * 64 + 63 > wq && ch * 64 < s_end && ch * 64 <= bound) {
          unsigned long long b = 0ull;
          for (int lane = 0; lane < 64; ++lane) {
            const int idx = ch * 64 + lane;
            if (idx < lim && idx > wq && (w.info[idx].x & DI_VALID) &&
                commit_conflict(q, qn, w.info[idx], (int)w.nb[idx].w, w.range2, w.far2, w.align2)) b |= 1ull << lane;
          }
          if (b) { const int o = ch * 64 + first_bit(b); s_end = o < s_end ? o : s_end; }
        }
    }
    s_wave[wv] = s_end;
  }
  int s_end = s_wave[0];
  for (int wv = 1; wv < WAVES; ++wv) s_end = s_wave[wv] < s_end ? s_wave[wv] : s_end;
  Outcome r{};
  r.cur_n = w.n;
  if (t_end < s_end) {
    const unsigned tf = w.info[t_end].x;
    if (tf & DI_FULL) { r.err = ERR_CELL; r.committed = t_end; }
    else if (tf & DI_HR) { r.cur_n -= 1; r.committed = t_end + 1; }
    else if (r.cur_n >= w.cap) { r.err = ERR_POINT; r.committed = t_end; }
    else { r.cur_n += 1; r.committed = t_end + 1; }
    *how = 3;
  } else {
    r.committed = s_end;
    if (s_end < lim && (w.info[s_end].x & DI_BAD)) r.err = ERR_BAD;
    *how = s_end == lim ? 0 : (s_end < first_inv ? 1 : 2);
  }
  for (int ch = 0; ch < NCH; ++ch) {
    r.mask[ch] = am[ch] & low_mask(r.committed - ch * 64);
    if (r.mask[ch]) r.any_commit = true;
  }
  for (int i = 0; i < r.committed; ++i) if ((w.info[i].x & DI_CHG) && (w.info[i].x & DI_NBOV)) r.any_apply = true;
  return r;
}

// ---- random windows
struct Rng {
  uint64_t s;
  uint64_t next() { s += 0x9e3779b97f4a7c15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
  double u() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
  bool p(double x) { return u() < x; }
};

static unsigned pack_xy(int x, int y) { return (unsigned)((x & 0xffff) | (y << 16)); }

static Window make_window(Rng &g) {
  Window w;
  static const int sizes[] = {1, 2, 7, 8, 63, 64, 65, 100, 128, 129, 192, 255, 256};
  w.lim = g.p(0.5) ? sizes[g.below(13)] : 1 + g.below(256);
  const int reach = 8 + g.below(40), cell = reach + g.below(16);       // the longest interaction range, the cell edge (px)
  w.range2 = reach * reach; w.far2 = 4 * reach * reach;
  const int al = 4 + g.below(reach); w.align2 = al * al;
  static const int fields[] = {48, 96, 256, 512, 1024, 4096};
  int field = fields[g.below(6)];
  if (field / cell > 255) field = 255 * cell;
  const int nslots = 4 << g.below(9);
  w.cap = 64 + g.below(64);
  w.n = g.p(0.3) ? w.cap - g.below(2) : 1 + g.below(w.cap);          // often at, or one below, the capacity
  // a kind of window per draw: few or many changing steps, invalid reports, births and deaths
  static const double pc_[] = {0.0, 0.01, 0.03, 0.1, 0.3, 0.8};
  const double p_chg = pc_[g.below(6)], p_inv = g.p(0.5) ? 0.0 : 0.002 * (1 << g.below(5)), p_bd = g.p(0.4) ? 0.0 : 0.02 * (1 << g.below(5));
  const double p_full = g.p(0.7) ? 0.0 : 0.05, p_resc = 0.1 * g.below(4), p_nb = 0.25 * g.below(4);
  w.info.resize(w.lim); w.nb.resize(w.lim);
  for (int i = 0; i < w.lim; ++i) {
    unsigned f = (unsigned)g.below(nslots);
    const bool valid = !g.p(p_inv);
    bool hr = true, ha = true;
    if (g.p(p_bd)) { hr = g.p(0.5); ha = !hr; }
    const int rx = g.below(field), ry = g.below(field);
    int ax = rx, ay = ry;
    if (!hr || g.p(0.5)) { ax = g.below(field); ay = g.below(field); }       // a jump, or a move of a few pixels (some cross a cell border)
    else { ax = rx + g.below(2 * reach + 1) - reach; ay = ry + g.below(2 * reach + 1) - reach; }
    ax = ax < 0 ? 0 : (ax >= field ? field - 1 : ax); ay = ay < 0 ? 0 : (ay >= field ? field - 1 : ay);
    if (valid) {
      f |= DI_VALID;
      if (hr) f |= DI_HR;
      if (ha) f |= DI_HA;
      const bool acc = g.p(0.5), chg = acc && g.p(2.0 * p_chg);
      if (acc) f |= DI_ACC;
      if (chg) {
        f |= DI_CHG;
        if (ha && g.p(p_full)) f |= DI_FULL;
        if (g.p(p_nb)) { f |= DI_NB; if (g.p(0.5)) { f |= DI_NB2; if (g.p(0.4)) f |= DI_NBOV; } }
      }
      if (g.p(p_resc)) f |= DI_RESC;
    } else if (!g.p(0.25)) f |= DI_BAD;                                       // (the kernel always sets it; the rule asks for the bit)
    w.info[i] = make_uint4(f, hr ? pack_xy(rx, ry) : 0u, ha ? pack_xy(ax, ay) : 0u,
                           (unsigned)((hr ? rx / cell : 0) | ((hr ? ry / cell : 0) << 8) | ((ha ? ax / cell : 0) << 16) | ((ha ? ay / cell : 0) << 24)));
    // neighbours within reach of the step's points, their radii, the step's own reach
    const int bx = ha ? ax : rx, by = ha ? ay : ry;
    unsigned nbw[2], nr[2];
    for (int k = 0; k < 2; ++k) {
      int x = bx + g.below(2 * reach + 1) - reach, y = by + g.below(2 * reach + 1) - reach;
      x = x < 0 ? 0 : x; y = y < 0 ? 0 : y;
      nbw[k] = pack_xy(x, y); nr[k] = (unsigned)g.below(reach);
    }
    w.nb[i] = make_uint4(nbw[0], nbw[1], nr[0] | (nr[1] << 8), (unsigned)(g.p(0.02) ? 255 : g.below(reach)));
  }
  return w;
}

int main(int argc, char **argv) {
  const int n_windows = argc > 1 ? atoi(argv[1]) : 60000;
  Rng g{12345};
  long long mismatches = 0, how_n[4] = {0, 0, 0, 0}, over8 = 0, errs[4] = {0, 0, 0, 0}, apply = 0;
  for (int it = 0; it < n_windows; ++it) {
    const Window w = make_window(g);
    int how = 0;
    const Outcome a = decide_serial(w), b = decide_split(w, &how);
    if (!(a == b)) {
      if (++mismatches <= 5)
        fprintf(stderr, "window %d (lim %d): serial committed %d err %d n %d, split committed %d err %d n %d\n", it, w.lim, a.committed,
                a.err, a.cur_n, b.committed, b.err, b.cur_n);
    }
    how_n[how] += 1; errs[a.err] += 1;
    int nchg = 0;
    for (int ch = 0; ch < NCH; ++ch) nchg += __builtin_popcountll(a.mask[ch]);
    if (nchg > 8) over8 += 1;
    if (a.any_apply) apply += 1;
  }
  printf("windows=%d mismatches=%lld end_none=%lld end_conflict=%lld end_invalid=%lld end_T=%lld committed_over8=%lld err_point=%lld err_cell=%lld err_bad=%lld any_apply=%lld\n",
         n_windows, mismatches, how_n[0], how_n[1], how_n[2], how_n[3], over8, errs[ERR_POINT], errs[ERR_CELL], errs[ERR_BAD], apply);
  return mismatches ? 1 : 0;
}
