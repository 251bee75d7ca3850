// layout_walk.hip -- host program of tests/test_layout_host.py: walks the pointer walkers of csrc/mpp_layout.hpp over host
// buffers of exactly the counted size and prints, per shape, the size and every array's offset, length and element size.
// Built for the host only, with -fsanitize=address,undefined: every array is written from its first to its last byte, so an
// array that leaves its buffer or a misaligned element ends the program.  It includes nothing but the layout header.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mpp_cnn_rs_object_detection_amd/csrc/mpp_layout.hpp"

struct Item { const void *p; size_t n, elem; };
template <class Inner>
struct Logged {               // a pointer walker that remembers what it handed out
  Inner in;
  std::vector<Item> items;
  explicit Logged(unsigned char *b) : in(b) {}
  template <class T> void add(T *f, size_t n) { items.push_back(Item{f, n, sizeof(T)}); }
  template <class T, class N> void take(T *&f, N n) { in.take(f, n); add(f, (size_t)n); }
  template <class T> void take_if(T *&f, int n) { in.take_if(f, n); add(f, (size_t)n); }
  template <class T, class N, class... U> void same(N n, T *&f, U *&...g) { in.same(n, f, g...); add(f, (size_t)n); (add(g, (size_t)n), ...); }
  void align16() { in.align16(); }
};

static int fail(const char *what) { fprintf(stderr, "layout_walk: %s\n", what); return 1; }

// names[i] / fields[i]: the arrays in memory order, as the struct names them; items: what the walk handed out, in its order
static int report(const unsigned char *buf, size_t n_names, const char *const *names, const void *const *fields,
                  const std::vector<Item> &items) {
  if (items.size() != n_names) return fail("the walk handed out another number of arrays than the struct has");
  for (size_t i = 0; i < n_names; ++i) {
    if (items[i].p != fields[i]) return fail("the walk's order is not the order of the names");
    const long long off = fields[i] ? (long long)((const unsigned char *)fields[i] - buf) : -1;
    printf(" %s=%lld:%zu:%zu", names[i], off, items[i].n, items[i].elem);
    if (fields[i]) memset((void *)fields[i], 0x5a, items[i].n * items[i].elem);
  }
  printf("\n");
  return 0;
}

static const char *const LDS_NAMES[] = {"s", "r", "a", "ca", "sa", "hl", "hw", "rad", "lin", "red0", "red1", "edges", "trig", "rowbase",
                                        "stash_v0", "stash_v1", "clip", "xy", "order", "cell_items", "cell_cnt", "stash_slot", "gate",
                                        "rec", "sh"};
static const char *const HBM_STATE_NAMES[] = {"s", "r", "a", "ca", "sa", "hl", "hw", "rad", "lin", "red0", "red1", "xy", "order",
                                              "cell_items", "cell_cnt", "gate"};
static const char *const HBM_LDS_NAMES[] = {"edges", "trig", "rowbase", "stash_v0", "stash_v1", "clip", "stash_slot", "rec", "sh"};
static const char *const DEEP_NAMES[] = {"pw", "tring", "racc", "clist", "info", "nb", "st", "poff", "tcnt", "ltab"};

int main() {
  const int caps[] = {1, 7, 64, 65, 1024, 65535}, cells[][2] = {{1, 1}, {9, 7}, {256, 64}, {64, 2048}};
  const int specs[] = {0, 1, 8, 16, 64}, rows[] = {0, 65, 1025}, waves_[] = {1, 4, 8, 16}, nmaxs[] = {8, 128, 256};
  printf("sizeof Rec=%zu uint4=%zu\n", sizeof(Rec), sizeof(uint4));
  for (int cap : caps) for (auto &ce : cells) for (int rb : rows) for (int waves : waves_) {
    const int ncell = ce[0], cell_cap = ce[1];
    for (int spec : specs) {                     // ---- the chain in LDS
      const size_t bytes = lds_bytes(cap, ncell, cell_cap, spec, rb, waves);
      unsigned char *buf = (unsigned char *)malloc(bytes);   // exactly the counted size: the sanitizer's red zone starts right behind it
      if (!buf || ((size_t)buf & 15)) return fail("malloc");
      Logged<LdsCursor> w(buf);
      Lds L;
      chain_layout(w, L, cap, ncell, cell_cap, spec, rb, waves);
      const Lds C = carve(buf, cap, ncell, cell_cap, spec, rb, waves);
      if (memcmp(&C, &L, sizeof L)) return fail("carve and the logged walk disagree");
      const void *const f[] = {L.s, L.r, L.a, L.ca, L.sa, L.hl, L.hw, L.rad, L.lin, L.red0, L.red1, L.edges, L.trig, L.rowbase,
                               L.stash_v0, L.stash_v1, L.clip, L.xy, L.order, L.cell_items, L.cell_cnt, L.stash_slot, L.gate, L.rec, L.sh};
      printf("chain cap=%d ncell=%d cell_cap=%d spec=%d rowbase_n=%d waves=%d bytes=%zu", cap, ncell, cell_cap, spec, rb, waves, bytes);
      if (report(buf, 25, LDS_NAMES, f, w.items)) return 1;
      free(buf);
    }
    for (int nmax : nmaxs) for (int ext = 0; ext < 2; ++ext) {   // ---- the deep rounds: the chain with spec 0, then the round's arrays
      const size_t base = deep_base_bytes(cap, ncell, cell_cap, rb, waves), bytes = base + deep_extra_bytes(nmax, waves, ext);
      unsigned char *buf = (unsigned char *)malloc(bytes);
      if (!buf || ((size_t)buf & 15)) return fail("malloc");
      Logged<LdsCursor> w0(buf);
      Lds L;
      chain_layout(w0, L, cap, ncell, cell_cap, 0, rb, waves);
      const void *const f0[] = {L.s, L.r, L.a, L.ca, L.sa, L.hl, L.hw, L.rad, L.lin, L.red0, L.red1, L.edges, L.trig, L.rowbase,
                                L.stash_v0, L.stash_v1, L.clip, L.xy, L.order, L.cell_items, L.cell_cnt, L.stash_slot, L.gate, L.rec, L.sh};
      if (nmax == nmaxs[0] && ext == 0) {
        printf("deep_chain cap=%d ncell=%d cell_cap=%d spec=0 rowbase_n=%d waves=%d bytes=%zu", cap, ncell, cell_cap, rb, waves, base);
        if (report(buf, 25, LDS_NAMES, f0, w0.items)) return 1;
      }
      Logged<ByteCursor> w(buf + base);
      DeepLds D;
      deep_layout(w, D, nmax, waves, ext);
      const DeepLds C = deep_carve(buf + base, nmax, waves, ext);
      if (memcmp(&C, &D, sizeof D)) return fail("deep_carve and the logged walk disagree");
      const void *const f[] = {D.pw, D.tring, D.racc, D.clist, D.info, D.nb, D.st, D.poff, D.tcnt, D.ltab};
      printf("deep cap=%d ncell=%d cell_cap=%d rowbase_n=%d waves=%d nmax=%d ext=%d base=%zu bytes=%zu", cap, ncell, cell_cap, rb, waves,
             nmax, ext, base, bytes);
      if (report(buf, 10, DEEP_NAMES, f, w.items)) return 1;
      free(buf);
    }
  }
  for (int cap : caps) for (auto &ce : cells) {     // ---- the HBM-state chain: its workspace slice
    const int ncell = ce[0], cell_cap = ce[1];
    const size_t bytes = hbm_state_bytes(cap, ncell, cell_cap);
    unsigned char *buf = (unsigned char *)aligned_alloc(HBM_ALIGN, bytes);
    if (!buf) return fail("aligned_alloc");
    Logged<HbmSlots> w(buf);
    Lds L;
    memset(&L, 0, sizeof L);
    hbm_state_layout(w, L, cap, ncell, cell_cap);
    const void *const f[] = {L.s, L.r, L.a, L.ca, L.sa, L.hl, L.hw, L.rad, L.lin, L.red0, L.red1, L.xy, L.order, L.cell_items, L.cell_cnt, L.gate};
    printf("hbm_state cap=%d ncell=%d cell_cap=%d bytes=%zu", cap, ncell, cell_cap, bytes);
    if (report(buf, 16, HBM_STATE_NAMES, f, w.items)) return 1;
    for (int spec : specs) for (int rb : rows) for (int waves : waves_) {   // ... and its LDS
      const size_t lbytes = hbm_lds_bytes(spec, rb, waves);
      unsigned char *lds = (unsigned char *)malloc(lbytes);
      if (!lds || ((size_t)lds & 15)) return fail("malloc");
      const Lds C = carve_hbm(lds, buf, cap, ncell, cell_cap, spec, rb, waves);
      Logged<LdsCursor> wl(lds);
      Lds M = L;
      hbm_lds_layout(wl, M, spec, rb, waves);
      if (memcmp(&C, &M, sizeof M)) return fail("carve_hbm and the logged walks disagree");
      const void *const g[] = {M.edges, M.trig, M.rowbase, M.stash_v0, M.stash_v1, M.clip, M.stash_slot, M.rec, M.sh};
      if (cap == caps[0] && ncell == cells[0][0]) {
        printf("hbm_lds spec=%d rowbase_n=%d waves=%d bytes=%zu", spec, rb, waves, lbytes);
        if (report(lds, 9, HBM_LDS_NAMES, g, wl.items)) return 1;
      }
      free(lds);
    }
    free(buf);
  }
  return 0;
}
