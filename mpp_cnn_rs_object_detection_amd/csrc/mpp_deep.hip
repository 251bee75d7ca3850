// mpp_deep.hip -- the "deep round" chain kernel: every LANE evaluates one speculative step.
//
// Same chain, same bits as mpp_chain_kernel (mpp_sampler.hip) -- the reference's loop rjmcmc.py:83-164 with the
// proposals drawn from Philox by step index -- organised for what the chain actually does after its first few thousand
// steps: of the ~25 % of proposals the Metropolis test accepts, four out of five re-write a point with the very values it
// already has (a data-driven transform that draws the class the mark sits in, a translation onto the same pixel), and
// only 2-5 % of all steps change the configuration.  A round of 8 steps, one wave each, is then almost always all
// rejects -- and costs a wave's latency per step.  Here a round is up to 64 * WAVES steps:
//   A  the kernel TYPE of each of the round's steps is a function of its Philox words alone; the steps are counting-
//      sorted by type across the workgroup so that the lanes of one wave run (mostly) the same kernel and do not
//      serialise on the draw;
//   B  every active lane draws and evaluates its step on its own against the round's start state (the lane forms of
//      draw_proposal / evaluate: the arithmetic, and its order, are those of the wave forms), decides it, and reports
//      (valid, changes-the-state, slot, positions) in 12 bytes of LDS;
//   C  every wave takes the same commit decision from those reports: steps commit in order; a committed change
//      invalidates the later steps that could have seen it (same slot, same cell, within 2 * max_inter) and the round ends
//      at the first invalid step; an accepted step that writes the bits that are already there changes nothing and ends
//      nothing.  The decision needs no order (mpp_commit.hpp): the changing steps are dealt to the waves, each wave tests
//      its steps against the later reports, and the first conflict any wave found ends the round;
//   D  the few lanes whose step commits with a change evaluate it a second time, writing the cached reductions of the
//      neighbours directly (no stash), and after a barrier move the point between cell lists and re-write its slot.
// The depth of a round follows the number of steps the last rounds committed.  Temperatures are a function of the step
// index alone: a ring in LDS holds those of the next steps, extended by as many entries as a round commits.
#include <cstdlib>

#ifdef MPP_DEEP_PROF
// diagnostic build only: cycles inside the draw of the data-driven translation (mpp_window.hpp), per wave, summed over the
// launch -- up to the window's total, from there to the row, from there to the column.  The empty asm makes the stamp wait
// for the value; the lanes of a wave that draw run the same instructions, the first of them adds the wave's cycles.  The
// kernel moves the sums into phase slots 20 .. 22 of its wave when it ends.
__device__ unsigned long long g_win_clk[16 * 3];
#define MPP_WIN_T0() unsigned long long wt_ = clock64()
#define MPP_WIN_STAMP(i, v)                                                                             \
  do {                                                                                                  \
    asm volatile("" ::"v"(v));                                                                          \
    const unsigned long long n_ = clock64();                                                            \
    if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) atomicAdd(&g_win_clk[(threadIdx.x >> 6) * 3 + (i)], n_ - wt_); \
    wt_ = n_;                                                                                           \
  } while (0)
#endif

#include "mpp_chain.hpp"
#include "mpp_commit.hpp"
#include "mpp_prepass.hpp"
#include "mpp_launch.hpp"

#define DEEP_NMAX_LIMIT 256      // most steps of one round (deeper rounds commit no more: the first conflict ends them)
#ifdef MPP_DEEP_PROF
// diagnostic build only (profiles/tools/build_deep_prof.sh): cycles of wave 0 per phase of a round, summed over the launch,
// in stats[16 + 24 * wave + phase]
#define DPH_N 24
#define DPH_T0() dph_t_ = clock64()
#define DPH(i) do { const unsigned long long n_ = clock64(); dph_[i] += n_ - dph_t_; dph_t_ = n_; } while (0)
#define DPH_ARGS , unsigned long long *dph_, unsigned long long &dph_t_
#define DPH_PASS , dph_, dph_t_
#else
#define DPH_T0()
#define DPH(i)
#define DPH_ARGS
#define DPH_PASS
#endif
// (the bits of a step report, DI_*, and the pair test of the commit decision: mpp_commit.hpp)

// ---- state mutation by ONE lane (energy_point_set.py:118-154); two steps that commit in the same round touch different
// cells and slots
__device__ __forceinline__ void cell_remove_1(const Chain &c, int cell, int slot) {
  const Lds &L = c.L;
  const int cnt = L.cell_cnt[cell];
  unsigned short *it = L.cell_items + (size_t)cell * c.h.cell_cap;
  int idx = -1;
  for (int i = 0; i < cnt; ++i) if (idx < 0 && it[i] == slot) idx = i;
  if (idx >= 0) {
    it[idx] = it[cnt - 1];
    L.cell_cnt[cell] = (unsigned short)(cnt - 1);
  }
}
__device__ __forceinline__ void cell_insert_1(const Chain &c, int cell, int slot) {
  const Lds &L = c.L;
  const int cnt = L.cell_cnt[cell];          // (room was checked when the step was chosen)
  L.cell_items[(size_t)cell * c.h.cell_cap + cnt] = (unsigned short)slot;
  L.cell_cnt[cell] = (unsigned short)(cnt + 1);
}
__device__ __forceinline__ void write_slot_1(const Chain &c, int slot, const Rec &q) {
  const Lds &L = c.L;
  L.xy[slot] = (q.ax & 0xffff) | (q.ay << 16);
  L.s[slot] = q.as; L.r[slot] = q.ar; L.a[slot] = q.aa;
  L.ca[slot] = q.ca; L.sa[slot] = q.sa; L.hl[slot] = q.hl; L.hw[slot] = q.hw; L.rad[slot] = q.rad;
  L.lin[slot] = q.lin_a; L.gate[slot] = (unsigned char)q.gate_a; L.red0[slot] = q.ra0; L.red1[slot] = q.ra1;
}

// evaluate() of mpp_chain.hpp in its lane form, in two halves around the ONE call of eval_delta_lane the kernel has (the
// step's evaluation and, for a step that commits, the second pass that writes the neighbours' reductions go through the
// same call site: with two, the inliner leaves a real call behind and the chain state lives in scratch memory)
__device__ __forceinline__ void deep_post(const Chain &c, Rec &r, int n, double T, bool tracing) {
  double fwd, bwd;
  green_terms(c.P, r, n, c.t.intensity, &fwd, &bwd);
  // rjmcmc.py:105-113 (one exp instead of three logs, see evaluate())
  double ratio = (bwd + EPS_GREEN) / (fwd + EPS_GREEN);
  r.accepted = ((r.u_acc + EPS_GREEN) < exp(-r.dE / T) * ratio) ? 1 : 0;
  if (tracing) { r.fwd = fwd; r.bwd = bwd; r.log_alpha = (-r.dE / T) + log(bwd + EPS_GREEN) - log(fwd + EPS_GREEN); }
}

// inclusive prefix sum over the 64 lanes (DPP: shifts within the rows of 16, then the two row broadcasts); EXEC must be full
__device__ __forceinline__ int wave_incl_scan(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);     // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);     // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);     // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);     // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     // row_bcast:31 -> rows 2, 3
  return v;
}

// clip_area_wave() for up to CLIP_SLOTS rectangle pairs at once: the wave works in groups of 16 lanes, lane li < 8 of a group
// owns vertex li of its group's polygon (the group's two polygon buffers are those of one clip slot).  Every vertex goes
// through exactly the arithmetic of clip_area() / clip_area_wave(), the shoelace sum runs in vertex order: the same bits.
// A data-driven birth lands on an object, i.e. on the rectangle that already sits there: nearly every birth asks for a
// clip, ten per wave and round -- one after the other they were a third of the neighbour evaluation.
// `gact`: my group has a pair; sx .. cy: its subject and clip corners (the same in all lanes of the group).
__device__ __forceinline__ double clip_area_groups(const Chain &c, bool gact, const double *sx, const double *sy, const double *cx,
                                                   const double *cy) {
  const int g = c.lane >> 4, li = c.lane & 15;
  double *buf = c.L.clip + ((size_t)c.wave * CLIP_SLOTS + g) * 32;
  double *ax = buf, *ay = buf + 8, *bx = buf + 16, *by = buf + 24;
  if (li < 4) {
    ax[li] = li == 0 ? sx[0] : (li == 1 ? sx[1] : (li == 2 ? sx[2] : sx[3]));
    ay[li] = li == 0 ? sy[0] : (li == 1 ? sy[1] : (li == 2 ? sy[2] : sy[3]));
  }
  wave_lds_fence();
  int na = gact ? 4 : 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    na = clip_edge_stage(li, 16 * g, 0xffffull, na, cx[e], cy[e], cx[(e + 1) & 3], cy[(e + 1) & 3], ax, ay, bx, by);
    double *tx = ax, *ty = ay;
    ax = bx; ay = by; bx = tx; by = ty;
    wave_lds_fence();
  }
  const bool valid = li < na;
  const int ii = valid ? li : 0, jj = ii + 1 >= na ? 0 : ii + 1;
  if (li < 8) bx[li] = valid ? ax[ii] * ay[jj] - ax[jj] * ay[ii] : 0.0;
  wave_lds_fence();
  double t_[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) t_[i] = bx[i];
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) if (i < na) s += t_[i];
  wave_lds_fence();
  return na < 3 ? 0.0 : 0.5 * fabs(s);
}

// The neighbours' part of dE for ALL steps a wave evaluates (energy_graph.py:139-225; the arithmetic of eval_delta<FAST>,
// mpp_chain.hpp, per neighbour, summed in the same order).  Lane i leads step i (`lead`: it has a point to remove and / or a
// rectangle to add).  One lane walking the 3 x 3 cells around its own step's points is a chain of dependent LDS reads per
// cell and entry (78 k cycles a round); here the work of all the wave's steps is dealt to all 64 lanes, twice:
//   1  the cells to look at -- the 3 x 3 block around a step's removed point, then, unless it is the same block, the one
//      around its added point -- go to the lanes, 128 at a time (two neighbouring cells per lane); a lane looks at its
//      cells' entries, four at a time, and keeps those within the longest interaction range of the removed or the added
//      point; an exclusive prefix sum puts them into the wave's candidate list in (step, cell, entry) order -- the order
//      eval_delta sums in;
//   2  the list goes to the lanes, 64 (step, neighbour) pairs at a time: the neighbour's geometry and cached reductions from
//      LDS, the step's added rectangle from its leader's registers (ds_bpermute); rectangle clips and the re-reduction of a
//      neighbour that loses its extremum are done by the whole wave, one after the other, as in eval_delta<FAST> (the
//      re-reduction is the function it calls, rereduce_wave of mpp_chain.hpp); the few neighbours whose energy changes are
//      added to their step's sum in list order; the reductions of the added point itself (max / min: order-free) are LDS
//      atomics on the bit patterns.
// `apply` (wave-uniform): the changed reductions are written to the caches (the second pass of a step that commits).
// Model: pair 0 = rectangle overlap / max, pair 1 = alignment / min (FAST).
template <bool EXT>
__device__ __forceinline__ void deep_delta(const Chain &c, const DeepLds &D, bool lead, bool has_rem, bool has_add, int rem,
                                           int rxy, int axy, double a_s, double a_r, double a_a, double a_hl, double a_hw,
                                           double a_ca, double a_sa, double a_rad, bool apply, double *sum_out, double *ra0_out,
                                           double *ra1_out, int *nchg_out, int *nb0_out, int *nb1_out, int *nbr_out, int *nresc_out, int *su_out, double *sv_out, bool *nonfinite_out DPH_ARGS) {
  const Lds &L = c.L;
  unsigned int *clist = D.clist + (size_t)c.wave * DEEP_CLIST;
  unsigned long long *racc = D.racc + (size_t)c.wave * (EXT ? 192 : 128);
  const int flags = (lead ? 4 : 0) | (lead && has_rem ? 1 : 0) | (lead && has_add ? 2 : 0);
  const int maxd2_0 = c.pr0.maxd2, maxd2_1 = c.pr1.maxd2, range2 = maxd2_0 > maxd2_1 ? maxd2_0 : maxd2_1;
  const double rew = c.pr1.p0 != 0.0 ? 1.0 : 0.0;
  const unsigned long long below = (1ull << c.lane) - 1ull;
  // the 3 x 3 blocks to look at: around the removed point, then -- unless it is the same block -- around the added one;
  // ptab lists them in (step, removed before added) order: lane | 0x80 for an added point's block
  unsigned char *ptab = D.ltab + (size_t)c.wave * 128;
  int npos = 0, ntasks = 0;
  {
    const int rcell_i = cell_coord(c, rxy & 0xffff), rcell_j = cell_coord(c, (rxy >> 16) & 0xffff);
    const int acell_i = cell_coord(c, axy & 0xffff), acell_j = cell_coord(c, (axy >> 16) & 0xffff);
    const bool pa_ = lead && has_rem, pb_ = lead && has_add && !(has_rem && rcell_i == acell_i && rcell_j == acell_j);
    const int cnt_ = (pa_ ? 1 : 0) + (pb_ ? 1 : 0);
    const int incl = wave_incl_scan(cnt_);
    int pos = incl - cnt_;
    if (pa_) ptab[pos++] = (unsigned char)c.lane;
    if (pb_) ptab[pos] = (unsigned char)(c.lane | 0x80);
    npos = __builtin_amdgcn_readlane(incl, 63);
    ntasks = 9 * npos;
  }
  racc[c.lane] = 0ull; racc[64 + c.lane] = 0ull;
  if (EXT) racc[128 + c.lane] = 0ull;
  wave_lds_fence();
  double sum = 0.0;
  int nchg = 0, M = 0, t0 = 0, nb0 = 0, nb1 = 0, nbr = 0, nresc = 0, su = 0;
  double sv00 = 0.0, sv01 = 0.0, sv10 = 0.0, sv11 = 0.0;       // new reductions of the first two neighbours that change
  bool pending = false;
  int p_cnt = 0, p_base[2] = {0, 0}, p_i[2] = {0, 0};
  unsigned long long p_mask[2] = {0ull, 0ull};
  for (;;) {
    bool final = false;
    if (__ballot(pending) == 0ull) {
      if (t0 >= ntasks) final = true;
      else {
        // ---- 1: the next 128 (block, cell) pairs, two neighbouring ones per lane
        p_cnt = 0;
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
          const int t = t0 + 2 * c.lane + q2;
          const int ip = (t * 7282) >> 16, k = t - 9 * ip;          // t / 9, t % 9 (t < 1152)
          const int pe = t < ntasks ? (int)ptab[ip] : 0;            // the block's step and kind
          const int i = pe & 63;
          const bool second = (pe & 0x80) != 0;
          const int sfl = __shfl(flags, i, WAVE), srem = __shfl(rem, i, WAVE), srxy = __shfl(rxy, i, WAVE), saxy = __shfl(axy, i, WAVE);
          const bool s_hr = sfl & 1, s_ha = sfl & 2;
          const int rx = srxy & 0xffff, ry = (srxy >> 16) & 0xffff, ax = saxy & 0xffff, ay = (saxy >> 16) & 0xffff;
          const int cir = cell_coord(c, rx), cjr = cell_coord(c, ry), cia = cell_coord(c, ax), cja = cell_coord(c, ay);
          const int k3 = (k * 11) >> 5;                              // k / 3 for k < 9
          const int ci = (second ? cia : cir) + k3 - 1, cj = (second ? cja : cjr) + (k - 3 * k3) - 1;
          bool ok = t < ntasks;
          if (ok && second && s_hr && abs(ci - cir) <= 1 && abs(cj - cjr) <= 1) ok = false;      // already listed
          ok = ok && ci >= 0 && ci < c.h.nx && cj >= 0 && cj < c.h.ny;
          const int cell = ok ? cj + ci * c.h.ny : 0;
          const int cnt = ok ? (int)L.cell_cnt[cell] : 0;
          const int base = cell * c.h.cell_cap;
          unsigned long long mask = 0ull;
          for (int e0 = 0; __ballot(e0 < cnt) != 0ull; e0 += 4) {
            int u_[4], xy_[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) u_[q] = e0 + q < cnt ? (int)L.cell_items[base + e0 + q] : 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) xy_[q] = e0 + q < cnt ? L.xy[u_[q]] : 0;
            if (EXT) {
              // a candidate neighbour (ANY entry of the cells looked at, as eval_delta's generic form does) whose own energy is
              // not finite makes the reference's E(after) - E(before) over the neighbourhood inf - inf = NaN
#pragma unroll
              for (int q = 0; q < 4; ++q)
                if (e0 + q < cnt && u_[q] != (s_hr ? srem : -1)) {
                  const double lu = L.lin[u_[q]];
                  if (!(lu - lu == 0.0)) racc[128 + i] = 1ull;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int ux = xy_[q] & 0xffff, uy = (xy_[q] >> 16) & 0xffff;
              const int dxr = ux - rx, dyr = uy - ry, dxa = ux - ax, dya = uy - ay;
              const bool inr = (s_hr && dxr * dxr + dyr * dyr <= range2) || (s_ha && dxa * dxa + dya * dya <= range2);
              if (e0 + q < cnt && u_[q] != (s_hr ? srem : -1) && inr) mask |= 1ull << (e0 + q);
            }
          }
          p_mask[q2] = mask; p_base[q2] = base; p_i[q2] = i;
          p_cnt += __popcll(mask);
        }
        t0 += 2 * WAVE;
        pending = p_cnt > 0;
        DPH(12);
      }
    }
    bool flush = final;
    if (!final) {
      // append the pairs of the waiting lanes, in lane order, as far as the list has room
      const int c_ = pending ? p_cnt : 0;
      const int incl = wave_incl_scan(c_);
      const bool fit = pending && M + incl <= DEEP_CLIST;
      const unsigned long long fm = __ballot(fit);
      if (fit) {
        int pos = M + incl - c_;
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
          unsigned long long m = p_mask[q2];
          while (m) {
            const int e = __ffsll((long long)m) - 1;
            m &= m - 1;
            clist[pos++] = ((unsigned int)p_i[q2] << 16) | (unsigned int)L.cell_items[p_base[q2] + e];
          }
        }
        pending = false;
      }
      if (fm) M = __builtin_amdgcn_readlane(M + incl, 63 - __clzll((long long)fm));
      flush = __ballot(pending) != 0ull;                   // what is left did not fit: evaluate the list first
      DPH(13);
    }
    if (flush && M > 0) {
      wave_lds_fence();
      // ---- 2: the list, 64 (step, neighbour) pairs at a time
      for (int j0 = 0; j0 < M; j0 += WAVE) {
        const int j = j0 + c.lane;
        const bool act = j < M;
        const unsigned int cu = act ? clist[j] : 0u;
        const int i = (int)(cu >> 16), u = (int)(cu & 0xffffu);
        const int sfl = __shfl(flags, i, WAVE), srem = __shfl(rem, i, WAVE), saxy = __shfl(axy, i, WAVE);
        const bool s_hr = act && (sfl & 1), s_ha = act && (sfl & 2);
        Geo2 ag;
        ag.g.x = saxy & 0xffff; ag.g.y = (saxy >> 16) & 0xffff;
        ag.g.hl = shfl_d(a_hl, i); ag.g.hw = shfl_d(a_hw, i); ag.g.ca = shfl_d(a_ca, i); ag.g.sa = shfl_d(a_sa, i);
        ag.rad = shfl_d(a_rad, i);
        Geo2 gr, gu;
        gr.g.x = gr.g.y = 0; gr.g.hl = gr.g.hw = gr.g.ca = gr.g.sa = 0.0; gr.rad = 0.0;
        gu = gr;
        double ov0 = 0.0, ov1 = 0.0;
        if (s_hr) gr = load_geo(L, srem);
        if (act) { gu = load_geo(L, u); ov0 = L.red0[u]; ov1 = L.red1[u]; }
        int d2r = 0, d2a = 0;
        if (s_hr) { const int dx = gu.g.x - gr.g.x, dy = gu.g.y - gr.g.y; d2r = dx * dx + dy * dy; }
        if (s_ha) { const int dx = gu.g.x - ag.g.x, dy = gu.g.y - ag.g.y; d2a = dx * dx + dy * dy; }
        // marks of the added rectangle: only the order of two rectangles on the same pixel asks for them
        const bool tie_a = s_ha && gu.g.x == ag.g.x && gu.g.y == ag.g.y;
        double sa_s = 0.0, sa_r = 0.0, sa_a = 0.0;
        if (__ballot(tie_a) != 0ull) { sa_s = shfl_d(a_s, i); sa_r = shfl_d(a_r, i); sa_a = shfl_d(a_a, i); }
        DPH(14);
        // -- overlaps first, in uniform control flow: every pair whose circumscribed circles meet is clipped by the wave
        const bool in_r0 = s_hr && d2r <= maxd2_0 && ov0 != 0.0, in_a0 = s_ha && d2a <= maxd2_0;
        const double Au = geo_area(gu.g);
        double ovl_r = 0.0, ovl_a = 0.0;
#pragma clang loop unroll(disable)
        for (int which = 0; which < 2; ++which) {
          const Geo2 gv = which == 0 ? gr : ag;
          bool need = which == 0 ? in_r0 : in_a0;
          double mn = 0.0;
          bool uf = false;
          if (need) {
            need = pair_needs_clip(Au, geo_area(gv.g), gu.rad + gv.rad, (double)(which == 0 ? d2r : d2a), &mn);
            if (need) {
              if (which == 0) uf = slot_first(L, u, gu.g, gv.g.x, gv.g.y, L.s[srem], L.r[srem], L.a[srem]);
              else uf = slot_first(L, u, gu.g, gv.g.x, gv.g.y, sa_s, sa_r, sa_a);
            }
          }
          double val = 0.0;
          unsigned long long m = __ballot(need);
          while (m) {                                              // CLIP_SLOTS pairs at a time, one per group of 16 lanes
            const int rank = __popcll(m & below);                  // my place among the lanes that still wait
            int my_src = -1;
#pragma unroll
            for (int k = 0; k < CLIP_SLOTS; ++k) {
              const int sk = m ? __ffsll((long long)m) - 1 : -1;
              if (m) m &= m - 1;
              if ((c.lane >> 4) == k) my_src = sk;
            }
            const bool gact = my_src >= 0;
            const int sl = gact ? my_src : 0;
            const Geo bu = shfl_geo(gu.g, sl), bv = shfl_geo(gv.g, sl);
            const bool u_first = __shfl((int)uf, sl, WAVE) != 0;
            double sx[4], sy[4], cx[4], cy[4];
            ordered_corners(u_first, bu, bv, sx, sy, cx, cy);
            const double area = clip_area_groups(c, gact, sx, sy, cx, cy);
            const double mine_ = shfl_d(area, (rank & (CLIP_SLOTS - 1)) << 4);
            if (need && rank < CLIP_SLOTS) { val = mine_ / (mn + AREA_EPS); need = false; }
          }
          if (which == 0) ovl_r = val; else ovl_a = val;
        }
        DPH(15);
        // -- the two reductions of the neighbour (MPP_PAIR_P of eval_delta)
        double nv0 = ov0, nv1 = ov1;
        bool resc0 = false, resc1 = false;
        if (act) {
          {                                                        // pair 0: overlap, max
            bool carries = false;
            if (in_r0) carries = ovl_r == ov0;
            if (in_a0 && ovl_a > 0.0) atomicMax(&racc[i], (unsigned long long)__double_as_longlong(ovl_a));
            if (carries) { if (in_a0 && ovl_a >= ov0) nv0 = ovl_a; else resc0 = true; }
            else if (in_a0) nv0 = ov0 > ovl_a ? ov0 : ovl_a;
          }
          {                                                        // pair 1: alignment, min
            const bool in_r1 = s_hr && d2r <= maxd2_1 && ov1 != 0.0, in_a1 = s_ha && d2a <= maxd2_1;
            bool carries = false;
            double v_add = 0.0;
            if (in_r1) carries = (1.0 - fabs(gu.g.ca * gr.g.ca + gu.g.sa * gr.g.sa) - rew) == ov1;
            if (in_a1) {
              v_add = 1.0 - fabs(gu.g.ca * ag.g.ca + gu.g.sa * ag.g.sa) - rew;
              if (v_add < 0.0) atomicMax(&racc[64 + i], (unsigned long long)__double_as_longlong(v_add));
            }
            if (carries) { if (in_a1 && v_add <= ov1) nv1 = v_add; else resc1 = true; }
            else if (in_a1) nv1 = ov1 < v_add ? ov1 : v_add;
          }
        }
        // -- a neighbour lost the point that carried its extremum and the added point does not take over: the wave
        //    re-reduces it over its own 3 x 3 cells (rereduce_wave, the function eval_delta<FAST> calls)
        unsigned long long rm = __ballot(resc0 || resc1);
        while (rm) {
          const int src = __ffsll((long long)rm) - 1;
          rm &= rm - 1;
          const bool need0 = __builtin_amdgcn_readlane((int)resc0, src) != 0, need1 = __builtin_amdgcn_readlane((int)resc1, src) != 0;
          const int us = __builtin_amdgcn_readlane(u, src), is = __builtin_amdgcn_readlane(i, src);
          if (c.lane == is) nresc += 1;
          const int rem_s = __builtin_amdgcn_readlane(srem, src);              // (the neighbour lost a removed point: has_rem)
          const bool ha_s = __builtin_amdgcn_readlane((int)s_ha, src) != 0;
          const Geo2 bu = readlane_geo2(gu, src);              // the neighbour, wave-uniform
          double acc0, acc1;
          rereduce_wave(c, us, bu, rem_s, need0, need1, maxd2_0, maxd2_1, rew, ha_s, ag, a_s, a_r, a_a, src, &acc0, &acc1, is);
          if (c.lane == src) {
            if (need0) nv0 = acc0;
            if (need1) nv1 = acc1;
          }
        }
        DPH(16);
        // -- the neighbours whose energy changes, added to their step's sum in list order
        const bool changed = act && (nv0 != ov0 || nv1 != ov1);
        double de = 0.0;
        if (changed) {
          const double lin = L.lin[u];
          const int gt = L.gate[u];
          de = finish_energy_c(c, lin + pair_part_c(c, gt, nv0, nv1)) - finish_energy_c(c, lin + pair_part_c(c, gt, ov0, ov1));
          if (apply) { L.red0[u] = nv0; L.red1[u] = nv1; }
        }
        unsigned long long cm = __ballot(changed);
        while (cm) {
          const int src = __ffsll((long long)cm) - 1;
          cm &= cm - 1;
          const int is = __builtin_amdgcn_readlane(i, src);
          const double v = readlane_d(de, src);
          const int uxy = __builtin_amdgcn_readlane((gu.g.x & 0xffff) | (gu.g.y << 16), src);
          const int uu = __builtin_amdgcn_readlane(u, src);
          const double w0 = readlane_d(nv0, src), w1 = readlane_d(nv1, src);
          const int ur = (int)ceil(readlane_d(gu.rad, src));          // its circumradius, rounded up
          if (c.lane == is) {
            sum += v;
            if (nchg == 0) { nb0 = uxy; nbr = ur & 0xff; su = uu; sv00 = w0; sv01 = w1; }
            else if (nchg == 1) { nb1 = uxy; nbr |= (ur & 0xff) << 8; su |= uu << 16; sv10 = w0; sv11 = w1; }
            nchg += 1;
          }
        }
        DPH(17);
      }
      M = 0;
      wave_lds_fence();
    }
    if (final) break;
  }
  wave_lds_fence();
  *sum_out = sum; *nchg_out = nchg; *nb0_out = nb0; *nb1_out = nb1; *nbr_out = nbr; *nresc_out = nresc;
  *su_out = su; sv_out[0] = sv00; sv_out[1] = sv01; sv_out[2] = sv10; sv_out[3] = sv11;
  *ra0_out = __longlong_as_double((long long)racc[c.lane]);
  *ra1_out = __longlong_as_double((long long)racc[64 + c.lane]);
  *nonfinite_out = EXT && racc[128 + c.lane] != 0ull;
}

// the state change of a committed step, done by the lane that evaluated it (n: the population at the round's start)
__device__ __forceinline__ void deep_mutate(const Chain &c, const Rec &r, int n, const double *st) {
  const Lds &L = c.L;
  int ci, cj;
  if (r.n_stash > 0 && r.n_stash <= 2) {               // the neighbours whose reductions change (more: the second pass wrote them)
    const int su = (int)__double_as_longlong(st[4]);
    L.red0[su & 0xffff] = st[0]; L.red1[su & 0xffff] = st[1];
    if (r.n_stash == 2) { L.red0[(su >> 16) & 0xffff] = st[2]; L.red1[(su >> 16) & 0xffff] = st[3]; }
  }
  if (r.has_rem && r.has_add) {                        // move / transform: same slot
    const int c0 = cell_index(c, r.rx, r.ry, &ci, &cj), c1 = cell_index(c, r.ax, r.ay, &ci, &cj);
    if (c0 != c1) { cell_remove_1(c, c0, r.tslot); cell_insert_1(c, c1, r.tslot); }
    write_slot_1(c, r.tslot, r);
  } else if (r.has_rem) {                              // death: last index takes the hole
    cell_remove_1(c, cell_index(c, r.rx, r.ry, &ci, &cj), r.tslot);
    const unsigned short last = L.order[n - 1];
    L.order[n - 1] = (unsigned short)r.tslot;
    L.order[r.tidx] = last;
  } else {                                             // birth: next free slot
    const int slot = L.order[n];
    cell_insert_1(c, cell_index(c, r.ax, r.ay, &ci, &cj), slot);
    write_slot_1(c, slot, r);
  }
}
// Does a move / transform propose the five values its target already holds?  Committing it writes the bits that are there:
// the cached geometry, unit energy and reductions are functions of those values.  The comparison is on the values (a mark
// that sits off the class edges differs from the edge of its own class); float ==: -0.0 equals 0.0, a NaN equals nothing.
__device__ __forceinline__ bool deep_same_values(const Lds &L, const Rec &r) {
  if (!(r.has_rem && r.has_add)) return false;
  const int sl = r.tslot;
  return r.ax == r.rx && r.ay == r.ry && r.as == L.s[sl] && r.ar == L.r[sl] && r.aa == L.a[sl];
}
// (QUE) the place of the report of the step at offset `off` of the round that starts at step `done`: by the step, so that a
// kept report is found by whichever lane gets its step in the next round (nmax: a power of two)
__device__ __forceinline__ int deep_slot(long long done, int off, int nmax) { return ((int)done + off) & (nmax - 1); }
__device__ __forceinline__ unsigned long long low_mask(int k) { return k <= 0 ? 0ull : (k >= 64 ? ~0ull : ((1ull << k) - 1ull)); }

// (QUE) The fields of a step that the neighbour pass does not read wait in LDS while it runs, in space of the step's own
// own that nothing else uses at that time: u_acc and qf in its report D.info[slot], qb in D.nb[slot] (both are written only
// after deep_post, and every wave has finished reading the previous round's reports before barrier (1)); lin_a and gate_a
// in D.pw[off] (the queue rounds sort nothing: no Philox words), where they stay until deep_mutate writes the slot.
__device__ __forceinline__ uint4 pack_dd(double a, double b) {
  const unsigned long long x = (unsigned long long)__double_as_longlong(a), y = (unsigned long long)__double_as_longlong(b);
  return make_uint4((unsigned)x, (unsigned)(x >> 32), (unsigned)y, (unsigned)(y >> 32));
}
__device__ __forceinline__ double unpack_d(unsigned lo, unsigned hi) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); }
// D.info and D.nb are indexed by the step (`slot`, see deep_slot), D.pw by the offset; the last word of D.pw[off] is the
// round's first_q of the report at that offset (carry_keeps, mpp_commit.hpp): none yet.
__device__ __forceinline__ void deep_park(const DeepLds &D, int slot, int off, const Rec &r) {
  D.info[slot] = pack_dd(r.u_acc, r.qf);
  D.nb[slot] = pack_dd(r.qb, 0.0);
  const uint4 l = pack_dd(r.lin_a, 0.0);
  D.pw[off] = make_uint4(l.x, l.y, (unsigned)r.gate_a, CARRY_NO_Q);
}
__device__ __forceinline__ void deep_unpark_green(const DeepLds &D, int slot, Rec &r) {
  const uint4 a = D.info[slot];
  const uint2 b = *(const uint2 *)(D.nb + slot);
  r.u_acc = unpack_d(a.x, a.y); r.qf = unpack_d(a.z, a.w); r.qb = unpack_d(b.x, b.y);
}
__device__ __forceinline__ void deep_unpark_unit(const DeepLds &D, int off, Rec &r) {
  const uint4 l = D.pw[off];
  r.lin_a = unpack_d(l.x, l.y); r.gate_a = (int)l.z;
}

// (QUE) the queues a wave serves: queue a, and for wave 1 queue b (wave 1: the uniform birth, a, and the uniform death, b;
// waves 4 and 5: the even and the odd entries of the data-driven translation's queue); ca / cb the position of the first
// entry not committed yet, ea / eb the end of the queue -- positions in the chain's part (reg) of pt.qoff / pt.qent;
// xa / xb the steps (offsets in the round) of my entries of queues a and b (or of the other parity), 0xffffffff past the end.
// Empty in the other instantiations: their code is the one they had before the queues.
template <bool Q> struct DeepQueues {};
template <> struct DeepQueues<true> {
  int qt_a, ca, ea, cb, eb;
  size_t reg;
  uint32_t xa, xb;
};

// EXT: the instantiation that knows the classic image energies (mpp_classics.hpp): every lane rasterises its own rectangle
// TAB: the births come from the pre-pass table `pt` (mpp_prepass.hip; not with EXT), and with eight waves the sorted steps
//      are dealt by cost
// QUE: (with TAB, eight waves, the cost deal) every wave takes its steps from the pre-pass queues of its kernel types, in the
//      same deal: no kernel type, no sort, no Philox block in the round (the round's window ends early where a wave would
//      have more than 64 steps)
// NCH: chunks of 64 step reports the commit decision keeps per lane (nmax <= 64 * NCH; the launcher picks it from nmax)
template <int WAVES, bool DIAG, int OCC, bool EXT, bool TAB, bool QUE = false, int NCH = DEEP_NMAX_LIMIT / 64>
__global__ __launch_bounds__(WAVE *WAVES, OCC) void mpp_deep_kernel(const DevParams Pv, const TileRef *tiles, int tile0,
                                                                 const long long *until, long long trace_base,
                                                                 unsigned long long seed, unsigned int chain0, int trace_tile,
                                                                 mpp_step_out *out, mpp_proposal *props, int nmax,
                                                                 int fixed_depth, int gain8, int flags,
                                                                 unsigned long long *stats, PreTab pt) {
  static_assert(!(TAB && EXT), "the pre-pass table is built for the instantiations without classic image energies");
  static_assert(!QUE || (TAB && WAVES == 8), "the queues are dealt to eight waves");
  const bool by_type = (gain8 & 0x100) == 0;      // (bit 8 of the gain word: deal the sorted steps in blocks instead -- A/B tests)
  const bool skip_opt = (flags & MPP_DEEP_SKIP_SAME) != 0;        // (option deep_skip_same)
  const bool carry_opt = QUE && (flags & MPP_DEEP_CARRY) != 0;    // (option deep_carry; the queue rounds only)
  gain8 &= 0xff;
  const DevParams *P = stage_params<(WAVES >= MPP_LDS_PARAMS_MIN_WAVES)>(Pv, WAVE * WAVES);
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int tile = tile0 + blockIdx.x;
  Chain c;
  c.P = P; c.t = tiles[tile];
  load_model_regs(c);
  load_hot(c);
  // the sizes behind every LDS address, from the kernel arguments and not from the staged copy of the block: a read of LDS
  // lands in vector registers, and the thirty-odd array bases derived from it would each hold one for the whole launch
  const int ncell = Pv.nx * Pv.ny, cap = Pv.cap;
  const int rowbase_n = Pv.rowbase_lds ? Pv.H + 1 : 0;
  c.L = carve(lds_raw, cap, ncell, Pv.cell_cap, 0, rowbase_n, WAVES);
  const DeepLds D = deep_carve(lds_raw + deep_base_bytes(cap, ncell, Pv.cell_cap, rowbase_n, WAVES), nmax, WAVES, EXT ? 1 : 0);
  c.lane = threadIdx.x & (WAVE - 1);
  c.wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const Lds &L = c.L;
  const int tid = threadIdx.x, nthr = WAVE * WAVES;
  const bool tracing = DIAG && (out != nullptr || props != nullptr) && tile == trace_tile;
  // A step that proposes the values its target already holds (deep_same_values) leaves the configuration as it is, accepted
  // or not, and in an untraced chain nothing reads its dE, its densities or its accept bit: such a step is not evaluated.
  // A traced chain records them for every step: it never skips.
  const bool skip_same = skip_opt && !tracing;
  // (QUE) A report behind the end of a round that no change the round committed conflicts with is the report the next round
  // would write again (carry_keeps, mpp_commit.hpp): phase C marks it DI_KEPT, and the lane that gets its step in the next
  // round leaves it as it is.  For a step to find its report whichever lane gets it, the queue rounds index D.info and D.nb
  // by the step (deep_slot: nmax is a power of two and a window has at most nmax steps), not by the offset in the round.
  // The bit is set by phase C alone, which re-writes it for all nmax entries every round: clear at launch, it is set on
  // entry to a round exactly for the kept reports of the round before.  A traced chain never keeps, as it never skips.
  const bool carry = carry_opt && !tracing;

  // ---------------------------------------------------------------- load the configuration (as mpp_chain_kernel does)
  int n0 = __builtin_amdgcn_readfirstlane(*c.t.n);
  int err = __builtin_amdgcn_readfirstlane(*c.t.err);
  if (n0 > cap) { n0 = cap; err = ERR_POINT_OVERFLOW; }
  for (int i = tid; i < 3 * MPP_NCLASS; i += nthr) L.edges[i] = P->maps.edges[i / MPP_NCLASS][i % MPP_NCLASS];
  for (int i = tid; i < MPP_NCLASS; i += nthr) {
    const double al = P->maps.edges[2][i] + MPP_PI / 2.0;
    L.trig[i] = cos(al); L.trig[MPP_NCLASS + i] = sin(al);
  }
  for (int i = tid; i < rowbase_n; i += nthr) L.rowbase[i] = c.t.rowbase[i];
  for (int i = tid; i < cap; i += nthr) L.order[i] = (unsigned short)i;
  for (int i = tid; i < ncell; i += nthr) L.cell_cnt[i] = 0;
  if constexpr (QUE) for (int i = tid; i < nmax; i += nthr) D.info[i].x = 0u;       // no report is kept
  __syncthreads();
  for (int i = tid; i < n0; i += nthr) {
    Rect q{c.t.px[i], c.t.py[i], c.t.ps[i], c.t.pr[i], c.t.pa[i]};
    Geo g = make_geo(q);
    double lin; int gate;
    unit_part<EXT>(P, c.t, L.edges, q, g, &lin, &gate, nullptr);
    L.xy[i] = (q.x & 0xffff) | (q.y << 16);
    L.s[i] = q.s; L.r[i] = q.r; L.a[i] = q.a; L.ca[i] = g.ca; L.sa[i] = g.sa; L.hl[i] = g.hl; L.hw[i] = g.hw;
    L.rad[i] = geo_radius(g);
    L.lin[i] = lin; L.gate[i] = (unsigned char)gate; L.red0[i] = 0.0; L.red1[i] = 0.0;
  }
  __syncthreads();
  const double alpha = c.t.T[1], T_target = c.t.T[2];
  const int rmask = 4 * nmax - 1;
  if (tid == 0) {                               // serial: keeps the cell order, hence the result, deterministic
    for (int i = 0; i < n0; ++i) {
      int xy = L.xy[i], ci, cj;
      int cell = cell_index(c, xy & 0xffff, (xy >> 16) & 0xffff, &ci, &cj);
      int cnt = L.cell_cnt[cell];
      if (cnt >= P->cell_cap) { err = ERR_CELL_OVERFLOW; break; }
      L.cell_items[(size_t)cell * P->cell_cap + cnt] = (unsigned short)i;
      L.cell_cnt[cell] = (unsigned short)(cnt + 1);
    }
    L.sh[1] = err;
  }
  if (tid == nthr - 1) {                        // temperatures of the first 2 * nmax steps (rjmcmc.py:158-159, one multiply per step)
    double Tc = *c.t.T;
    long long d0 = 0;                           // (QUE) the ring is indexed by the step's offset from the table's first
    if constexpr (QUE) d0 = pt.base ? *c.t.step - pt.base[blockIdx.x] : 0;
    for (int i = 0; i < 2 * nmax; ++i) { D.tring[(int)((d0 + i) & (long long)rmask)] = Tc; if (Tc > T_target) Tc *= alpha; }
  }
  __syncthreads();
  err = __builtin_amdgcn_readfirstlane(L.sh[1]);
  {                                             // cached pair reductions of the initial configuration
    Rect dummy{0, 0, 0, 0, 0};
    Geo2 dg;
    dg.g = Geo{0, 0, 0, 0, 0, 0}; dg.rad = 0.0;
    for (int u = tid; u < n0; u += nthr) {
      Geo2 gu = load_geo(L, u);
#pragma clang loop unroll(disable)
      for (int p = 0; p < P->model.n_pair; ++p) {
        double v;
        [[clang::always_inline]] v = rescan_lane(c, p, u, gu, -1, false, dummy, dg);     // (a real call pins the chain state in scratch)
        if (p == 0) L.red0[u] = v; else L.red1[u] = v;
      }
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- the chain
  // (QUE) A launch may start in mid-table -- after the hot start's handover, after a capacity stop: step0 is then the table's
  // first step and done starts at the chain's offset from it, so the round loop indexes the table as ever.
  long long done = 0;
  if constexpr (QUE) done = pt.base ? *c.t.step - pt.base[blockIdx.x] : 0;
  const long long step0 = *c.t.step - done;
  const long long n_steps = until[tile] - step0;
  const long long tr0 = step0 - trace_base;
  const unsigned long long seed_t = c.t.key_on ? (unsigned long long)c.t.key_seed : seed;
  const uint32_t chain_t = c.t.key_on ? c.t.key_chain : chain0 + (uint32_t)tile;
  const uint32_t k0 = (uint32_t)seed_t, k1 = (uint32_t)(seed_t >> 32);
  const unsigned long long below = (1ull << c.lane) - 1ull;
  int n = n0;                                   // the population, tracked by every wave
  int depth = WAVES, ema16 = WAVES * 16;        // steps of the next round; committed steps per round, x16, smoothed
  unsigned long long st_rounds = 0, st_eval = 0, st_apply = 0;
#ifdef MPP_DEEP_PROF
  unsigned long long dph_[DPH_N] = {0}, dph_t_ = 0, dph_fresh = 0;      // (dph_fresh: steps this wave evaluated afresh)
#endif

  // The loop alternates between two stages that share the call of eval_delta_lane: stage 1 draws and evaluates a round's
  // steps and decides which commit; stage 0 (only after a round with a change) applies them.
  int stage = 1;
  Rec r;
  r.valid = 0; r.kernel = 0; r.accepted = 0; r.has_rem = r.has_add = 0; r._pad = 0; r.tslot = -1; r.tidx = -1;
  r.ax = r.ay = r.rx = r.ry = 0; r.as = r.ar = r.aa = 0.0; r.hl = r.hw = r.ca = r.sa = r.rad = 0.0; r.lin_a = 0.0; r.gate_a = 1;
  bool mine = false, my_commit = false;
  int myoff = 0, lim = 0, committed = 0, cur_n = n, nb0 = 0, nb1 = 0, nbr = 0, ring_todo = 0;
  long long ring_from = 0;
  DeepQueues<QUE> qs;                           // (QUE) the wave's cursors into the queues
  if constexpr (QUE) {
    const int w = c.wave;
    qs.qt_a = w == 0 ? MPP_K_DBIRTH : w == 1 ? MPP_K_UBIRTH : w == 2 ? MPP_K_DDEATH : w == 3 ? MPP_K_GTRANS
            : w <= 5 ? MPP_K_DTRANS : w == 6 ? MPP_K_DTRANSF : MPP_K_GTRANSF;
    const unsigned int *qc = pt.qcnt + (size_t)blockIdx.x * MPP_NKERNEL * pt.qnblk;
    const int qend = (int)pt.qtot[blockIdx.x];
    qs.ca = __builtin_amdgcn_readfirstlane((int)qc[(size_t)qs.qt_a * pt.qnblk]);
    qs.ea = __builtin_amdgcn_readfirstlane(qs.qt_a + 1 < MPP_NKERNEL ? (int)qc[(size_t)(qs.qt_a + 1) * pt.qnblk] : qend);
    qs.cb = __builtin_amdgcn_readfirstlane((int)qc[(size_t)MPP_K_UDEATH * pt.qnblk]);
    qs.eb = __builtin_amdgcn_readfirstlane((int)qc[(size_t)(MPP_K_UDEATH + 1) * pt.qnblk]);
    qs.reg = (size_t)blockIdx.x * (size_t)pt.stride;
    qs.xa = qs.xb = 0xffffffffu;
    if (done > 0) {
      // the cursors start at the first entry of their queue that is not below `done`: the scanned counts give the position at
      // the enclosing block of PRE_BLOCK steps, a pass over that block's entries the rest (once, before the round loop)
      const size_t blk = (size_t)(done / PRE_BLOCK);
      auto first_at = [&](int qt, int end) {
        const int p0 = (int)qc[(size_t)qt * pt.qnblk + blk];
        int cnt = 0;
        for (int j = 0; j < PRE_BLOCK; j += WAVE) {
          const int i = p0 + j + c.lane;
          cnt += __popcll(__ballot(i < end && pt.qoff[qs.reg + i] < (uint32_t)done));
        }
        return __builtin_amdgcn_readfirstlane(p0 + cnt);
      };
      qs.ca = first_at(qs.qt_a, qs.ea);
      qs.cb = first_at(MPP_K_UDEATH, qs.eb);
    }
  }
  while (stage == 0 || (done < n_steps && err == 0)) {
    bool do_eval = my_commit && r.n_stash > 2;  // stage 0: the steps that commit and change more neighbours than they could note
    bool same = false;                          // stage 1: my step re-writes its target unchanged and is not evaluated (skip_same)
    DPH_T0();
    if (stage == 1) {
    int N = fixed_depth > 0 ? fixed_depth : depth;
    if (N > nmax) N = nmax;
    const int Lw = N / WAVES;                   // active lanes per wave
    const long long left = n_steps - done;
    lim = left < (long long)N ? (int)left : N;
    if constexpr (QUE) {
      int kq = 0;                               // my kernel type
      QEnt qe;                                  // my entry
      qe.off = 0u; qe.w2 = 0u; qe.u_acc = 0.0; qe.a = 0.0; qe.b = 0.0;
      // ---- A: my entries, and where the round's window must end for every wave to have at most 64 steps
      const uint32_t d32 = (uint32_t)done;
      const bool pair = c.wave == 4 || c.wave == 5;
      const int ia = pair ? qs.ca + 2 * c.lane + (c.wave == 5 ? 1 : 0) : qs.ca + c.lane;
      const int ib = pair ? qs.ca + 2 * c.lane + (c.wave == 5 ? 0 : 1) : qs.cb + c.lane;
      qs.xa = ia < qs.ea ? pt.qoff[qs.reg + ia] - d32 : 0xffffffffu;
      qs.xb = (pair || c.wave == 1) && ib < (pair ? qs.ea : qs.eb) ? pt.qoff[qs.reg + ib] - d32 : 0xffffffffu;
      if (c.wave != 1 && ia < qs.ea) qe = pt.qent[qs.reg + ia];
      uint32_t cut = (uint32_t)lim;
      if (c.wave == 1) {
        const uint32_t a63 = (uint32_t)__builtin_amdgcn_readlane((int)qs.xa, 63), b63 = (uint32_t)__builtin_amdgcn_readlane((int)qs.xb, 63);
        if (a63 < cut) cut = a63 + 1u;
        if (b63 < cut) cut = b63 + 1u;
        if (__popcll(__ballot(qs.xa < cut)) + __popcll(__ballot(qs.xb < cut)) > WAVE) {       // (then 32 of each at most)
          const uint32_t a32 = (uint32_t)__builtin_amdgcn_readlane((int)qs.xa, 32), b32 = (uint32_t)__builtin_amdgcn_readlane((int)qs.xb, 32);
          cut = min(cut, min(a32, b32));
        }
      } else {
        const uint32_t last = (uint32_t)__builtin_amdgcn_readlane((int)(c.wave == 4 ? qs.xb : qs.xa), 63);   // (a pair: entry 127)
        if (last < cut) cut = last + 1u;
      }
      if (c.lane == 0) D.tcnt[c.wave] = (unsigned short)cut;
      DPH(0);
      __syncthreads();                          // (1) also: the changes of the previous round are in place
      DPH(1);
      uint32_t lq = (uint32_t)lim;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) lq = min(lq, (uint32_t)D.tcnt[w]);
      lim = (int)lq;
      mine = qs.xa < lq;
      kq = qs.qt_a;
      myoff = (int)qs.xa;
      if (c.wave == 1) {                        // lanes [0, na) the uniform births, [na, na + nb) the uniform deaths
        const int na = __popcll(__ballot(qs.xa < lq)), nb = __popcll(__ballot(qs.xb < lq));
        const int d = c.lane - na;
        mine = c.lane < na + nb;
        kq = c.lane < na ? MPP_K_UBIRTH : MPP_K_UDEATH;
        const int iq = c.lane < na ? qs.ca + c.lane : qs.cb + d;
        if (mine) { qe = pt.qent[qs.reg + iq]; myoff = (int)(qe.off - d32); }
      }
      if (!mine) myoff = 0;
      DPH(2);
      // ---- B: evaluate my step (the TAB path below, its head from the entry instead of Philox words)
      // (every field anew, also in the lanes without a step: nothing of the last round's step stays live through the draw)
      r.valid = 0; r.kernel = 0; r.accepted = 0; r.has_rem = r.has_add = 0; r.tslot = -1; r.tidx = -1;
      r.ax = r.ay = r.rx = r.ry = 0; r.pid = -1; r.ncls = -1; r.acls = 0; r.n_stash = 0; r._pad2 = 0; r.gate_a = 1;
      r.as = r.ar = r.aa = r.aux0 = r.aux1 = r.u_acc = r.qf = r.qb = r.dE = 0.0;
      r.hl = r.hw = r.ca = r.sa = r.rad = r.lin_a = r.ra0 = r.ra1 = 0.0;
      const int myslot = deep_slot(done, myoff, nmax);
      // (a kept report: the lane behaves as one whose step re-writes its target unchanged, and leaves the report untouched)
      if (mine && carry && (D.info[myslot].x & DI_KEPT)) same = true;
      else if (mine) {
        r.valid = 1;
        int keep = 0;
        const bool pre_b = kq == MPP_K_UBIRTH || kq == MPP_K_DBIRTH;      // a birth: the table has it all
        if (pre_b) deep_load_birth(pt, qe.w2, kq, r);
        else draw_tail_q(c, kq, qe, n, r, &keep);
        DPH(3);
        if (r.valid && r.has_add && (r.ax < 0 || r.ax >= c.h.H || r.ay < 0 || r.ay >= c.h.W)) { r.valid = 0; r.kernel = -1; }
        same = skip_same && r.valid && deep_same_values(L, r);
        if (r.valid && !pre_b && !same) {
          const MapVals pmv{0.f, 0.f, 0.f, 0.f, 0.0, 0.0, 0.0, 0};
          deep_add_geo(c, r, keep);
          deep_pre<false>(c, r, keep, tracing, pmv, nullptr);
        }
        if (!same) deep_park(D, myslot, myoff, r);
      }
      if (carry && same) D.pw[myoff].w = CARRY_NO_Q;      // (an evaluated lane parked it)
#ifdef MPP_DEEP_PROF
      if (stats) { const int nf = __popcll(__ballot(mine && !(same && r.valid == 0))); if (c.lane == 0) dph_fresh += (unsigned long long)nf; }
#endif
      do_eval = mine && r.valid && (r.has_rem || r.has_add) && !same;
      DPH(4);
    } else {
    const bool act0 = c.lane < Lw;
    const int e = c.wave * Lw + c.lane;         // my offset when the types are computed, my sorted position afterwards

    // ---- A: kernel type of step done + e, counting sort by type over the workgroup
    int kt = 15;
    uint32_t w0[4] = {0u, 0u, 0u, 0u};
    uint32_t pword = 0u;                        // (TAB) the step's word of the pre-pass table, requested here, used after (1)
    if (act0 && e < lim) {
      const uint64_t s = (uint64_t)(step0 + done + e);
      philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), 0u, chain_t, k0, k1, w0);
      const double uk = u53(w0[0], w0[1]);
      kt = 0;
      while (kt < P->n_kernels - 1 && P->p_cum[kt] <= uk) ++kt;
      if (TAB && (kt == MPP_K_UBIRTH || kt == MPP_K_DBIRTH)) pword = pt.word[(size_t)blockIdx.x * pt.stride + done + e];
    }
    unsigned long long same_kt = 0ull;
    int cnt_lane = 0;                           // lane k: steps of type k in this wave
#pragma unroll
    for (int k = 0; k < MPP_NKERNEL; ++k) {
      const unsigned long long m = __ballot(kt == k);
      if (kt == k) same_kt = m;
      if (c.lane == k) cnt_lane = __popcll(m);
    }
    const int rank = __popcll(same_kt & below);
    if (c.lane < 16) D.tcnt[c.wave * 16 + c.lane] = (unsigned short)cnt_lane;
    DPH(0);
    __syncthreads();                            // (1) also: the changes of the previous round are in place
    DPH(1);
    int tot = 0, pre = 0;
    if (c.lane < 16) {
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        const int v = D.tcnt[w * 16 + c.lane];
        if (w < c.wave) pre += v;
        tot += v;
      }
    }
    int excl = 0, run = 0;
#pragma unroll
    for (int k = 0; k < MPP_NKERNEL; ++k) {
      const int t_k = __builtin_amdgcn_readlane(tot, k);
      if (c.lane == k) excl = run;
      run += t_k;
    }
    const int first = __shfl(excl + pre, kt & 15, WAVE);
    if (kt != 15) {
      const int p = first + rank;
      // (TAB: a birth reads none of its words past the type: word 2 carries its ordinal in the table instead)
      if (TAB && (kt == MPP_K_UBIRTH || kt == MPP_K_DBIRTH)) w0[2] = pword >> 4;
      D.pw[p] = make_uint4(w0[0], w0[1], w0[2], w0[3]);
      D.poff[p] = (unsigned short)e;
    }
    __syncthreads();                            // (2)
    DPH(2);

    // ---- B: evaluate my step.  Sorted position e of the thread: with eight waves and the eight kernels of the mixture, wave w
    //      takes the steps of kernel w (it then runs ONE kernel's code, not the tail of one type and the head of the next);
    //      otherwise -- or should a type have more than 64 steps -- the sorted steps are dealt to the waves in blocks.
    int es = e;
    mine = act0 && e < lim;
    if (TAB && WAVES == 8 && by_type) {
      // by cost (profiles/prepass.md; cycles of a round's wave before barrier (3)).  With the births' draw in the table, the
      // data-driven transform is the slowest kernel by far -- its draw and its neighbour pass: its steps go to two waves,
      // split in sorted order; the two uniform kernels share a wave; every other kernel keeps a wave of its own.  Waves w
      // and w + 4 share a SIMD: each of the two transform halves shares it with a light wave (the data-driven birth,
      // the uniform pair), wave 0 -- it extends the temperature ring -- gets the lightest.
      int t_[MPP_NKERNEL];
#pragma unroll
      for (int k = 0; k < MPP_NKERNEL; ++k) t_[k] = __builtin_amdgcn_readlane(tot, k);
      // sorted segments: [0, b1) uniform birth + death, [b1, b2) data-driven birth, [b2, b3) data-driven death,
      // [b3, b4) Gaussian translation, [b4, b5) and [b5, b6) the data-driven translation, [b6, b7) Gaussian transform,
      // [b7, b8) data-driven transform
      const int b1 = t_[MPP_K_UBIRTH] + t_[MPP_K_UDEATH], b2 = b1 + t_[MPP_K_DBIRTH], b3 = b2 + t_[MPP_K_DDEATH];
      const int b4 = b3 + t_[MPP_K_GTRANS], b5 = b4 + (t_[MPP_K_DTRANS] + 1) / 2, b6 = b4 + t_[MPP_K_DTRANS];
      const int b7 = b6 + t_[MPP_K_GTRANSF], b8 = b7 + t_[MPP_K_DTRANSF];
      const bool fits = b8 == lim && b1 <= WAVE && b2 - b1 <= WAVE && b3 - b2 <= WAVE && b4 - b3 <= WAVE && b5 - b4 <= WAVE &&
                        b6 - b5 <= WAVE && b7 - b6 <= WAVE && b8 - b7 <= WAVE;
      if (fits) {
        // wave:     0   1   2   3   4   5   6   7
        // segment: b1  0   b2  b3  b4  b5  b7  b6   (its first position)
        const int w = c.wave;
        const int lo = w == 0 ? b1 : w == 1 ? 0 : w == 2 ? b2 : w == 3 ? b3 : w == 4 ? b4 : w == 5 ? b5 : w == 6 ? b7 : b6;
        const int hi = w == 0 ? b2 : w == 1 ? b1 : w == 2 ? b3 : w == 3 ? b4 : w == 4 ? b5 : w == 5 ? b6 : w == 6 ? b8 : b7;
        mine = c.lane < hi - lo;
        es = lo + c.lane;
      }
    } else if (WAVES == 8 && by_type && !EXT) {           // (EXT: the contrast terms are evaluated one rectangle at a time per wave -- equal shares)
      bool fits = true;
#pragma unroll
      for (int k = 0; k < MPP_NKERNEL; ++k) {
        const int t_k = __builtin_amdgcn_readlane(tot, k);
        fits = fits && t_k <= WAVE && (k < WAVES || t_k == 0);
      }
      if (fits) {
        const int first_w = __builtin_amdgcn_readlane(excl, c.wave), tot_w = __builtin_amdgcn_readlane(tot, c.wave);
        mine = c.lane < tot_w;
        es = first_w + c.lane;
      }
    }
    myoff = mine ? (int)D.poff[es] : 0;
    r.valid = 0; r.kernel = 0; r.accepted = 0; r.has_rem = r.has_add = 0; r.tslot = -1; r.tidx = -1;
    r.ax = r.ay = r.rx = r.ry = 0; r.pid = -1; r.ncls = -1; r.acls = 0; r.n_stash = 0; r._pad2 = 0; r.gate_a = 1;      // (as in the queue rounds)
    r.as = r.ar = r.aa = r.aux0 = r.aux1 = r.u_acc = r.qf = r.qb = r.dE = 0.0;
    r.hl = r.hw = r.ca = r.sa = r.rad = r.lin_a = r.ra0 = r.ra1 = 0.0;
    int keep_x = 0;                                    // (EXT only: what deep_pre needs after the cooperative pass below)
    MapVals pmv_x{0.f, 0.f, 0.f, 0.f, 0.0, 0.0, 0.0, 0};
    if (mine) {
      r.valid = 1;
      int keep = 0;
      MapVals pmv{0.f, 0.f, 0.f, 0.f, 0.0, 0.0, 0.0, 0};
      uint32_t w[8];
      const uint4 wv = D.pw[es];
      w[0] = wv.x; w[1] = wv.y; w[2] = wv.z; w[3] = wv.w;
      const uint64_t s = (uint64_t)(step0 + done + myoff);
      bool pre_b = false;                      // (TAB) a birth: the table has it all
      if (TAB) {
        const double uk = u53(w[0], w[1]);
        int k = 0;
        while (k < P->n_kernels - 1 && P->p_cum[k] <= uk) ++k;
        pre_b = k == MPP_K_UBIRTH || k == MPP_K_DBIRTH;
        if (pre_b) deep_load_birth(pt, w[2], k, r);
      }
      if (!pre_b) {
        philox4x32_10((uint32_t)s, (uint32_t)(s >> 32), 1u, chain_t, k0, k1, w + 4);
        draw_proposal<true, !TAB>(c, w, n, r, &keep, k0, k1, s, chain_t, &pmv);
      }
      DPH(3);
      if (r.kernel >= MPP_K_SPLIT) { r.valid = 0; r.kernel = -1; }
      if (r.valid && r.has_add && (r.ax < 0 || r.ax >= c.h.H || r.ay < 0 || r.ay >= c.h.W)) { r.valid = 0; r.kernel = -1; }
      same = skip_same && r.valid && deep_same_values(L, r);
      if (r.valid && !pre_b && !same) {
        deep_add_geo(c, r, keep);
        if (!EXT) deep_pre<EXT>(c, r, keep, tracing, pmv, nullptr);
      }
      if (EXT) { keep_x = keep; pmv_x = pmv; }
    }
    // the classic contrast term of every rectangle this wave's steps add: one rectangle at a time by the whole wave
    // (csrc/mpp_classics.hpp: rows, then columns, across lanes), before the lanes go their own ways again
    double cpre = 0.0;
    bool have_cpre = false;
    if (EXT) {
      int cterm = -1;
      for (int k = 0; k < P->model.n_unit; ++k) if (P->model.unit[k].kind == MPP_U_CONTRAST) cterm = k;
      if (cterm >= 0) {
        unsigned long long m = __ballot(mine && r.valid && r.has_add && !same);
        while (m) {
          const int l = __ffsll((long long)m) - 1;
          m &= m - 1;
          Geo g;
          g.x = __builtin_amdgcn_readlane(r.ax, l); g.y = __builtin_amdgcn_readlane(r.ay, l);
          g.hl = readlane_d(r.hl, l); g.hw = readlane_d(r.hw, l); g.ca = readlane_d(r.ca, l); g.sa = readlane_d(r.sa, l);
          const double v = classic_contrast_wave(P->model.unit[cterm], c.t.img, c.t.img_c, c.h.H, c.h.W, g, c.lane);
          if (c.lane == l) { cpre = v; have_cpre = true; }
        }
      }
    }
    if (EXT && mine && r.valid && !same) deep_pre<EXT>(c, r, keep_x, tracing, pmv_x, have_cpre ? &cpre : nullptr);
    do_eval = mine && r.valid && (r.has_rem || r.has_add) && !same;
    DPH(4);
    }
    }
    // ---- the neighbours' part of dE (energy_graph.py:139-225) for all steps of the wave; stage 0 writes their cached
    //      reductions
    {
      double ra0 = 0.0, ra1 = 0.0, sde = 0.0, sv[4];
      int ns = 0, nresc = 0, su = 0;
      bool nonf = false;
      const bool hr = r.has_rem != 0, ha = r.has_add != 0;
      deep_delta<EXT>(c, D, do_eval, hr, ha, hr ? r.tslot : -1, (r.rx & 0xffff) | (r.ry << 16), (r.ax & 0xffff) | (r.ay << 16), r.as,
                 r.ar, r.aa, r.hl, r.hw, r.ca, r.sa, r.rad, stage == 0, &sde, &ra0, &ra1, &ns, &nb0, &nb1, &nbr, &nresc, &su, sv, &nonf DPH_PASS);
      if (stage == 1 && do_eval) {
        double dE = sde;
        if constexpr (QUE) deep_unpark_unit(D, myoff, r);
        if (ha) dE += finish_energy_c(c, r.lin_a + pair_part_c(c, r.gate_a, ra0, ra1));
        if (hr) dE -= finish_energy_c(c, L.lin[r.tslot] + pair_part_c(c, (int)L.gate[r.tslot], L.red0[r.tslot], L.red1[r.tslot]));
        if (EXT && nonf) dE = nan("");
        r.dE = dE; r.ra0 = ra0; r.ra1 = ra1; r.n_stash = ns; r._pad2 = nresc;
        if (ns > 0 && ns <= 2) {                 // (kept for the commit: written by this lane again, read by no other)
          double *st = D.st + (size_t)5 * myoff;
          st[0] = sv[0]; st[1] = sv[1]; st[2] = sv[2]; st[3] = sv[3]; st[4] = __longlong_as_double((long long)su);
        }
      }
    }
    DPH(stage == 1 ? 5 : 9);
    if (stage == 1) {
    const int myslot = QUE ? deep_slot(done, myoff, nmax) : myoff;       // where my report goes
    // (a lane that did not evaluate re-reads the bit: no flag of its own lives through the neighbour pass)
    if (mine && !(carry && same && (D.info[myslot].x & DI_KEPT))) {
      // the step's temperature: its ring entry stays as it is while the step is in the window (the ring is filled two rounds ahead)
      const double Tm = D.tring[(int)((done + myoff) & (long long)rmask)];
      // (a skipped step: nothing was parked for it, and no test is made.  Its report below is the one an evaluated re-write
      // gets, whichever way its test goes -- no DI_CHG, hence no DI_FULL / DI_NB*; no DI_RESC, for its added rectangle has the
      // removed one's bits and takes every extremum over; the reach radius from the target's cache, r.rad being 0 -- except
      // for DI_ACC, which the commit decision does not read: the bit stays clear, r.accepted is 0 from the round's reset.)
      if (!same) {
        if constexpr (QUE) deep_unpark_green(D, myslot, r);
        if (r.valid) deep_post(c, r, n, Tm, tracing);
      }
      // does the step change the configuration?  An accepted move that writes the values the slot already holds does not
      // (its cached geometry, unit energy and reductions are functions of those values: the same bits)
      bool chg = r.valid && r.accepted && (r.has_rem || r.has_add);
      if (chg && deep_same_values(L, r)) chg = false;
      bool full = false;
      if (chg && r.has_add) {
        int ci, cj;
        const int c1 = cell_index(c, r.ax, r.ay, &ci, &cj), c0 = r.has_rem ? cell_index(c, r.rx, r.ry, &ci, &cj) : -1;
        full = c1 != c0 && (int)L.cell_cnt[c1] >= c.h.cell_cap;
      }
      int ci_r = 0, cj_r = 0, ci_a = 0, cj_a = 0;
      if (r.has_rem) cell_index(c, r.rx, r.ry, &ci_r, &cj_r);
      if (r.has_add) cell_index(c, r.ax, r.ay, &ci_a, &cj_a);
      const int f = (r.tslot & 0xffff) | (r.valid ? DI_VALID : DI_BAD) | (chg ? DI_CHG : 0) | (r.has_rem ? DI_HR : 0) |
                    (r.has_add ? DI_HA : 0) | (r.accepted ? DI_ACC : 0) | (full ? DI_FULL : 0) | (chg && r.n_stash > 0 ? DI_NB : 0) |
                    (chg && r.n_stash > 1 ? DI_NB2 : 0) | (chg && r.n_stash > 2 ? DI_NBOV : 0) | (r.valid && r._pad2 > 0 ? DI_RESC : 0);
      D.info[myslot] = make_uint4((unsigned)f, (unsigned)((r.rx & 0xffff) | (r.ry << 16)), (unsigned)((r.ax & 0xffff) | (r.ay << 16)),
                                 (unsigned)(ci_r | (cj_r << 8) | (ci_a << 16) | (cj_a << 24)));
      // circumradius (rounded up, at most 255) of the largest rectangle the step removes or adds: how far its overlap term reaches
      double rr = r.has_add ? r.rad : 0.0;
      if (r.has_rem) { const double r0_ = L.rad[r.tslot]; rr = r0_ > rr ? r0_ : rr; }
      const int own_r = rr < 254.0 ? (int)ceil(rr) : 255;
      D.nb[myslot] = make_uint4((unsigned)nb0, (unsigned)nb1, (unsigned)nbr, (unsigned)own_r);
    }
    // temperatures of the steps that entered the window with the PREVIOUS round's commit (the ring is two rounds ahead; wave 0
    // runs the cheapest kernels and would wait at the barrier anyway): one multiply per step, in step order, as the chain does
    if (tid == WAVE - 1 && ring_todo > 0) {
      double Tc = D.tring[(int)((ring_from - 1) & (long long)rmask)];
      for (int i = 0; i < ring_todo; ++i) {
        if (Tc > T_target) Tc *= alpha;
        D.tring[(int)((ring_from + i) & (long long)rmask)] = Tc;
      }
    }
    ring_todo = 0;
    DPH(6);
    __syncthreads();                            // (3)
    DPH(7);

    // ---- C: which steps commit (every wave takes the same decision from the same reports; the rule and the pair test:
    //      mpp_commit.hpp).  Steps commit in order; a committed move / transform q makes a later report o untrustworthy
    //      when o read something q writes (commit_conflict).  The round ends at the first report that is invalid or that
    //      a changing step before it conflicts with (s_end) -- or before that, at the first changing step that is a birth /
    //      death or finds its cell full (t_end).  No pair test depends on the outcome of another: the changing steps that
    //      can move s_end are dealt to the waves, each wave keeps the first report ITS steps conflict with, and the
    //      minimum over the waves is s_end.
    uint4 o_[NCH];
    int or_[NCH];                               // reach radius of the report's rectangles
    unsigned long long am_[NCH];                // the changing steps
    const int nch = (lim + 63) >> 6;            // chunks in use
    int first_inv = lim, t_end = lim;           // the first invalid report, the first changing step that ends the round
#pragma unroll
    for (int ch = NCH - 1; ch >= 0; --ch) {
      o_[ch] = make_uint4(0u, 0u, 0u, 0u); or_[ch] = 0; am_[ch] = 0ull;
      if (ch < nch) {
        const int idx = ch * 64 + c.lane;
        const bool in = idx < lim;
        const int sl = QUE ? deep_slot(done, idx, nmax) : idx;
        if (in) { o_[ch] = D.info[sl]; or_[ch] = (int)D.nb[sl].w; }
        const unsigned f = o_[ch].x;
        am_[ch] = __ballot(in && (f & DI_CHG));
        const unsigned long long bm = __ballot(in && !(f & DI_VALID)), tm = __ballot(in && commit_terminal(f));
        if (bm) first_inv = ch * 64 + __ffsll((long long)bm) - 1;
        if (tm) t_end = ch * 64 + __ffsll((long long)tm) - 1;
      }
    }
    committed = 0; cur_n = n;
    const int range2 = c.pr0.maxd2 > c.pr1.maxd2 ? c.pr0.maxd2 : c.pr1.maxd2, far2 = P->conflict_d2;
    // report i's flags (i < lim), from the chunk registers
    auto flags_at = [&](int i) {
      unsigned f = 0u;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) if ((i >> 6) == ch) f = (unsigned)__builtin_amdgcn_readlane((int)o_[ch].x, i & 63);
      return f;
    };
    // the changing steps that can move s_end: those below both ends (a conflict found by a later one lies beyond them)
    const int bound = t_end < first_inv ? t_end : first_inv;
    int nrel = 0;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) nrel += __popcll(am_[ch] & low_mask(bound - ch * 64));
    int s_end = first_inv;
    if (nrel > 0) {
      // the k-th of them goes to wave k % WAVES.  (Also a single one: letting every wave test it itself saves the barrier,
      // but measures no faster on the bench tile -- profiles/commit_split.md -- and costs the two-wave instantiation a
      // dword of scratch.)
      const bool deal = WAVES > 1;
      int cur = 0;
      for (int k = 0; k < nrel; ++k) {
        int wq = -1;
#pragma unroll
        for (int ch = NCH - 1; ch >= 0; --ch) {
          const unsigned long long t = am_[ch] & ~low_mask(cur - ch * 64) & low_mask(bound - ch * 64);
          if (t) wq = ch * 64 + __ffsll((long long)t) - 1;
        }
        cur = wq + 1;
        if (deal && (k & (WAVES - 1)) != c.wave) continue;
        // q's report from the lane that holds it (no LDS read whose address waits for the ballots); its neighbour word
        // is in no register: one broadcast read
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          if ((wq >> 6) == ch)
            q = make_uint4((unsigned)__builtin_amdgcn_readlane((int)o_[ch].x, wq & 63), (unsigned)__builtin_amdgcn_readlane((int)o_[ch].y, wq & 63),
                           (unsigned)__builtin_amdgcn_readlane((int)o_[ch].z, wq & 63), (unsigned)__builtin_amdgcn_readlane((int)o_[ch].w, wq & 63));
        const uint4 qn = D.nb[QUE ? deep_slot(done, wq, nmax) : wq];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          // (the chunks behind q; for the end of the round not beyond what is known to end it; for the kept reports all of
          // them: every report q conflicts with notes the lowest such q in its first_q word)
          const bool for_end = ch * 64 < s_end && ch * 64 <= bound;
          if (ch < nch && ch * 64 + 63 > wq && (for_end || carry)) {
            const int idx = ch * 64 + c.lane;
            bool bad = false;
            if (idx > wq && (o_[ch].x & DI_VALID)) bad = commit_conflict(q, qn, o_[ch], or_[ch], range2, far2, c.pr1.maxd2);
            if constexpr (QUE) { if (carry && bad) atomicMin(&D.pw[idx].w, (unsigned)wq); }
            const unsigned long long b = __ballot(bad);
            if (for_end && b) { const int o = ch * 64 + __ffsll((long long)b) - 1; s_end = o < s_end ? o : s_end; }
          }
        }
      }
      if constexpr (WAVES > 1) {
        if (deal) {
          // The waves' minima meet in L.sh[8 + wave].  The round loop has no other use for L.sh (the kernel reads sh[1]
          // once, before the loop), so the only writer of these words is this line, and between two of its executions
          // every wave passes the barrier below and then (1) and (3) of the next round: a wave cannot write its word for the
          // next round while a slow one still reads this round's -- whichever way the fast one leaves C, into the next
          // round's A or into stage 0.  nrel is the same in every wave: they all take the barrier or none does.
          DPH(18);
          if (c.lane == 0) L.sh[8 + c.wave] = s_end;
          __syncthreads();                      // (5)
          DPH(19);
#pragma unroll
          for (int w = 0; w < WAVES; ++w) {
            const int v = __builtin_amdgcn_readfirstlane(L.sh[8 + w]);
            s_end = v < s_end ? v : s_end;
          }
        }
      }
    }
    if (t_end < s_end) {                        // the commit reaches step t_end: it decides
      // capacity checks BEFORE anything of the step is applied: the chain stops in the state before it (see mpp_sampler.hip)
      // (the evaluating lane looked at the cell's count: no state is read here, see "stage")
      const unsigned tf = flags_at(t_end);
      if (tf & DI_FULL) { err = ERR_CELL_OVERFLOW; committed = t_end; }
      else if (tf & DI_HR) { cur_n -= 1; committed = t_end + 1; }             // death / birth: ends the round (n and order[] change)
      else if (cur_n >= cap) { err = ERR_POINT_OVERFLOW; committed = t_end; }
      else { cur_n += 1; committed = t_end + 1; }
    } else {
      committed = s_end;
      if (s_end < lim && (flags_at(s_end) & DI_BAD)) err = ERR_BAD_TARGET;
      // otherwise: invalidated by an earlier commit of this round -> evaluated again next round
    }
    if constexpr (QUE) {
      // the kept reports of the next round: wave ch re-writes the bit of chunk ch, in and behind the window (a window may be
      // shorter than the one before).  A round without a relevant changing step has no barrier (5) -- it commits its whole
      // window, or ends at a birth / death, or stops the chain, and has nothing to keep that a later round would use: a wave
      // that still loads its chunks sees the bit either way, and nothing in this phase reads it.  (first_q: the words are
      // complete after barrier (5), and without one nothing was noted.)
      if (carry) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          if (c.wave == ch && ch * 64 < nmax) {
            const int idx = ch * 64 + c.lane;
            unsigned *w = &D.info[deep_slot(done, idx, nmax)].x;
            if (idx < lim) {
              const unsigned of = o_[ch].x;
              bool keep = false;
              if (idx >= committed) keep = carry_keeps(of, idx, committed, s_end, cur_n != n, D.pw[idx].w);
              const unsigned nf = keep ? (of | DI_KEPT) : (of & ~(unsigned)DI_KEPT);
              if (nf != of) *w = nf;
            } else if (idx < nmax) {
              const unsigned of = *w;
              if (of & DI_KEPT) *w = of & ~(unsigned)DI_KEPT;
            }
          }
      }
    }
    bool any_commit = false, any_apply = false;     // a step commits with a change; ... and changes reductions of neighbours
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const unsigned long long cm = am_[ch] & low_mask(committed - ch * 64);      // the changing steps that commit
      if (cm) {
        any_commit = true;
        if (__ballot((o_[ch].x & DI_NBOV) != 0u) & cm) any_apply = true;
      }
    }

    if constexpr (QUE) {                        // the entries the round committed leave the queues
      const uint32_t cm = (uint32_t)committed;
      const int na = __popcll(__ballot(qs.xa < cm)), nb = __popcll(__ballot(qs.xb < cm));
      if (c.wave == 1) { qs.ca += na; qs.cb += nb; }
      else qs.ca += na + nb;                    // (nb: the other parity of a pair, 0 elsewhere)
    }

    // ---- D: apply the committed changes
    my_commit = false;
    if (mine) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) if ((myoff >> 6) == ch) my_commit = myoff < committed && ((am_[ch] >> (myoff & 63)) & 1ull);
    }
    if (DIAG && tracing && mine && myoff < committed) {
      const long long idx = tr0 + done + myoff;
      if (out) {
        mpp_step_out so;
        so.dE = r.dE; so.fwd = r.fwd; so.bwd = r.bwd; so.log_alpha = r.log_alpha;
        so.T = D.tring[(int)((done + myoff) & (long long)rmask)];
        so.accepted = r.accepted; so.n_after = (my_commit && !(r.has_rem && r.has_add)) ? cur_n : n;
        out[idx] = so;
      }
      if (props) {
        mpp_proposal pp;
        pp.kernel = r.kernel; pp.target = r.has_rem ? r.tidx : -1; pp.ax = r.ax; pp.ay = r.ay; pp.as = r.as;
        pp.ar = r.ar; pp.aa = r.aa; pp.aux0 = r.aux0; pp.aux1 = r.aux1; pp.param_id = r.pid;
        pp.new_class = r.ncls; pp.u_accept = r.u_acc;
        props[idx] = pp;
      }
    }
    DPH(8);
    if (stats) { st_rounds += 1; st_eval += (unsigned long long)lim; if (any_apply) st_apply += 1; }
    // depth of the next round: a multiple (gain8 / 8, default 2) of what the last rounds committed
    ema16 += committed - (ema16 >> 4);
    {
      int want = ((ema16 * gain8) >> 7) + WAVES;  // gain8 / 8 * mean + WAVES
      want = (want + WAVES - 1) / WAVES * WAVES;
      depth = want < WAVES ? WAVES : (want > nmax ? nmax : want);
    }
    // A committed step that changes reductions of its neighbours is evaluated a second time (stage 0).  When none does, the
    // lists and slots change right here: nothing between barrier (3) and the next round's barrier (1) reads them (the commit
    // decision above works on the reports alone).
    if (any_apply) stage = 0;                   // (my_commit of the steps without such neighbours: they just skip the pass)
    else {
      if (any_commit && my_commit) {
        if constexpr (QUE) deep_unpark_unit(D, myoff, r);
        deep_mutate(c, r, n, D.st + (size_t)5 * myoff);
      }
      my_commit = false;
      ring_from = done + 2 * nmax; ring_todo = committed;
      done += committed;
      n = cur_n;
    }
    } else {
      // ---- D: the committed changes (stage 0; their neighbours' reductions were written just above)
      __syncthreads();                          // (4) every reduction is written before a list or a slot changes
      DPH(10);
      if (my_commit) {
        if constexpr (QUE) deep_unpark_unit(D, myoff, r);
        deep_mutate(c, r, n, D.st + (size_t)5 * myoff);
      }
      my_commit = false;
      ring_from = done + 2 * nmax; ring_todo = committed;
      done += committed;
      n = cur_n;
      stage = 1;
      DPH(11);
    }
  }
  __syncthreads();

  // ---------------------------------------------------------------- write the configuration back
  for (int i = tid; i < n; i += nthr) {
    int slot = L.order[i], xy = L.xy[slot];
    c.t.px[i] = xy & 0xffff; c.t.py[i] = (xy >> 16) & 0xffff;
    c.t.ps[i] = L.s[slot]; c.t.pr[i] = L.r[slot]; c.t.pa[i] = L.a[slot];
  }
#ifdef MPP_DEEP_PROF
  if (c.lane == 0) for (int i = 0; i < 3; ++i) dph_[20 + i] = atomicExch(&g_win_clk[c.wave * 3 + i], 0ull);   // (one chain per launch: the probe's)
  if (stats && c.lane == 0) for (int i = 0; i < DPH_N; ++i) atomicAdd(stats + 16 + DPH_N * c.wave + i, dph_[i]);
  if (stats && c.lane == 0) atomicAdd(stats + 4, dph_fresh);
#endif
  if (tid == 0) {
    long long start = 0;                        // (QUE) where in the table this launch started
    if constexpr (QUE) start = *c.t.step - step0;
    *c.t.n = n; *c.t.err = err; *c.t.step = step0 + done;
    *c.t.T = D.tring[(int)(done & (long long)rmask)];
    if (stats) { atomicAdd(stats, st_rounds); atomicAdd(stats + 1, st_eval); atomicAdd(stats + 2, st_apply); atomicAdd(stats + 3, (unsigned long long)(done - start)); }
  }
}

// ---- host-side launcher ----------------------------------------------------------------------------
extern "C" size_t mpp_deep_lds_bytes(int cap, int ncell, int cell_cap, int rowbase_n, int waves, int nmax, int ext) {
  return deep_base_bytes(cap, ncell, cell_cap, rowbase_n, waves) + deep_extra_bytes(nmax, waves, ext);
}

template <int WAVES, bool DIAG, int OCC, bool EXT, bool TAB, bool QUE = false, int NCH = DEEP_NMAX_LIMIT / 64>
static hipError_t launch_deep_d(const ChainLaunch &a, int nmax, int fixed_depth, int gain8, int flags,
                                unsigned long long *stats, const PreTab &pt) {
  if (nmax > 64 * NCH || (nmax & (nmax - 1))) return hipErrorInvalidValue;     // (a power of two: the ring's mask, deep_slot)
  hipError_t e = hipFuncSetAttribute((const void *)mpp_deep_kernel<WAVES, DIAG, OCC, EXT, TAB, QUE, NCH>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((mpp_deep_kernel<WAVES, DIAG, OCC, EXT, TAB, QUE, NCH>), dim3(a.grid), dim3(WAVE * WAVES), a.lds, a.st, *a.P, a.tiles,
                     a.tile0, a.until, a.trace_base, a.seed, a.chain0, a.trace_tile, a.out, a.props, nmax, fixed_depth, gain8, flags, stats, pt);
  return hipGetLastError();
}

// waves = waves per chain (1, 2, 4, 8); nmax = most steps of one round (a power of two, waves <= nmax <= 64 * waves, <= 256);
// ext: a classic image energy among the unit terms (built for 1 and 8 waves, like the one-wave-per-step kernels)
// pt: the launch's birth table (mpp_prepass.hip), or pt->word == nullptr: the chains draw their births themselves; with
// pt->qoff, eight waves and the cost deal (gain8 without bit 8), the rounds take their steps from the table's queues
// flags: MPP_DEEP_SKIP_SAME: an untraced chain does not evaluate the steps that re-write their target unchanged (option
// deep_skip_same); MPP_DEEP_CARRY: an untraced chain in queue rounds keeps the reports behind a round's end that stay
// trustworthy, and does not evaluate their steps again (option deep_carry)
// (a.tape is not read: deep rounds draw their proposals from Philox)
extern "C" hipError_t mpp_launch_deep(const ChainLaunch &a, int waves, int occ, int nmax, int fixed_depth, int gain8, int flags,
                                      unsigned long long *stats, int ext, const PreTab *pt) {
  const bool diag = a.out || a.props, tab = pt->word != nullptr && !ext;
  // GO_(W, O, X, T[, Q, N]): that instantiation, traced or not
#define GO_(W, ...)                                                                                        \
  return diag ? launch_deep_d<W, true, __VA_ARGS__>(a, nmax, fixed_depth, gain8, flags, stats, *pt)               \
              : launch_deep_d<W, false, __VA_ARGS__>(a, nmax, fixed_depth, gain8, flags, stats, *pt)
  if (tab && pt->qoff != nullptr && waves == 8 && (gain8 & 0x100) == 0) {
    // the queue rounds keep two chunks of step reports per lane where the round has at most 128 steps (the default depth), four above
    if (nmax <= 128) { GO_(8, 2, false, true, true, 2); }
    GO_(8, 2, false, true, true, DEEP_NMAX_LIMIT / 64);
  }
#define GO(W, O, X) do { if (!(X) && tab) { GO_(W, O, false, true); } GO_(W, O, X, false); } while (0)
  if (ext) {
    switch (waves) {
      case 1: GO_(1, 1, true, false);
      case 8: GO_(8, 2, true, false);
    }
    return hipErrorNotSupported;
  }
  switch (waves) {
    case 1: if (occ >= 2) { GO(1, 2, false); } GO(1, 1, false);
    case 2: if (occ >= 2) { GO(2, 2, false); } GO(2, 1, false);
    case 4: if (occ >= 2) { GO(4, 2, false); } GO(4, 1, false);
    case 8: GO(8, 2, false);
  }
#undef GO
#undef GO_
  return hipErrorInvalidValue;
}
