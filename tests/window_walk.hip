// window_walk.hip -- host program of tests/test_window_rows_host.py: the draw of the data-driven translation
// (csrc/mpp_window.hpp, window_draw_rows: the function the kernels call) through both of its forms -- the rows' sums formed
// from the per-row prefix table, and read from the transposed table rowwin -- on small maps, at every pixel, for draws at
// the ends of [0, 1) and on the walk's own partial sums.  The tables are built here with the header's index and bound
// arithmetic, in vectors of exactly the sizes the library allocates, so that -fsanitize=address,undefined sees every
// index the draw forms.  Prints maps=, draws=, segs=, over17= (draws whose window has more than 17 rows), exact= (draws
// at which u * tot is bitwise a partial sum of the walk), mismatches=; the exit status is 1 when a draw or an entry differs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mpp_cnn_rs_object_detection_amd/csrc/mpp_window.hpp"

struct Map {
  int H, W;
  std::vector<float> det;
};
struct Tables {
  std::vector<double> rowpart, boxsum, rowwin;
};

static uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, 8); return b; }

// k_row_partial, k_boxsum and k_rowwin of csrc/mpp_maps.hip, one map
static Tables build(const Map &m, int md) {
  const int H = m.H, W = m.W;
  Tables t;
  t.rowpart.resize((size_t)H * W); t.boxsum.resize((size_t)H * W); t.rowwin.assign(rowwin_count(1, H, W), 0.0);
  for (int r = 0; r < H; ++r) {
    double s = 0.0;
    for (int j = 0; j < W; ++j) { s += (double)m.det[(size_t)r * W + j]; t.rowpart[(size_t)r * W + j] = s; }
  }
  for (int x = 0; x < H; ++x)
    for (int y = 0; y < W; ++y) {
      const WinBox b = window_box(x, y, md, H, W);
      double s = 0.0;
      for (int r = b.x0; r < b.x1; ++r) s += window_row_seg(t.rowpart.data() + (size_t)r * W, b.y0, b.y1);
      t.boxsum[(size_t)x * W + y] = s;
      t.rowwin[rowwin_index(x, y, H)] = window_row_seg(t.rowpart.data() + (size_t)x * W, b.y0, b.y1);
    }
  return t;
}

static Map make_map(int H, int W, int kind) {
  Map m{H, W, std::vector<float>((size_t)H * W)};
  uint32_t s = 12345u + 977u * H + 31u * W;
  for (int x = 0; x < H; ++x)
    for (int y = 0; y < W; ++y) {
      s = s * 1664525u + 1013904223u;
      float v = (float)(s >> 8) * (1.0f / 16777216.0f);          // kind 0: values in [0, 1)
      if (kind == 1) v = 1.0f;                                     // all ones: every partial sum is an integer, u * tot hits them exactly
      if (kind == 2) v = (x % 3 == 1 || y % 4 == 2) ? 0.0f : 1.0f; // all-zero rows and columns: equal partial sums, rows of weight 0
      m.det[(size_t)x * W + y] = v;
    }
  return m;
}

int main() {
  const int shapes[5][2] = {{1, 1}, {1, 40}, {40, 1}, {12, 20}, {33, 47}};
  const int mds[3] = {1, 8, 12};
  const double below_one = std::nextafter(1.0, 0.0);
  long maps = 0, draws = 0, segs = 0, over17 = 0, exact = 0, mismatches = 0;
  for (int si = 0; si < 5; ++si)
    for (int kind = 0; kind < 3; ++kind)
      for (int mi = 0; mi < 3; ++mi) {
        const int H = shapes[si][0], W = shapes[si][1], md = mds[mi];
        const Map m = make_map(H, W, kind);
        const Tables t = build(m, md);
        ++maps;
        const double *rp = t.rowpart.data(), *bs = t.boxsum.data(), *rw = t.rowwin.data();
        for (int x = 0; x < H; ++x)
          for (int y = 0; y < W; ++y) {
            const WinBox b = window_box(x, y, md, H, W);
            const int nrow = b.x1 - b.x0, wc = b.y1 - b.y0;
            // the rows' sums, entry against expression, bit for bit
            for (int r = b.x0; r < b.x1; ++r) {
              ++segs;
              if (bits(rw[rowwin_index(r, y, H)]) != bits(window_row_seg(rp + (size_t)r * W, b.y0, b.y1))) {
                ++mismatches;
                fprintf(stderr, "seg %dx%d kind %d md %d at (%d,%d) row %d\n", H, W, kind, md, x, y, r);
              }
            }
            // the draws: the two ends of [0, 1), and every u for which u * tot is a partial sum of the walk -- after each
            // row, and after each pixel of each row -- where the division gives such a u
            const double tot = bs[(size_t)x * W + y];
            std::vector<double> us = {0.0, below_one, 0.5};
            double before = 0.0;
            for (int r = b.x0; r < b.x1; ++r) {
              const double *row = rp + (size_t)r * W;
              const double lead = b.y0 > 0 ? row[b.y0 - 1] : 0.0;
              for (int j = 0; j < wc; ++j) {
                const double part = before + (row[b.y0 + j] - lead);
                if (tot > 0.0 && part < tot) us.push_back(part / tot);
              }
              before += window_row_seg(row, b.y0, b.y1);
              if (tot > 0.0 && before < tot) us.push_back(before / tot);
            }
            for (double u : us) {
              int ax = -1, ay = -1, bx = -2, by = -2;
              window_draw_rows(rp, bs, (const double *)nullptr, H, W, md, x, y, u, &ax, &ay);
              window_draw_rows(rp, bs, rw, H, W, md, x, y, u, &bx, &by);
              ++draws;
              if (nrow > MPP_WIN_ROWS || wc > MPP_WIN_ROWS) ++over17;
              // (is the threshold one of the walk's partial sums, bitwise?)
              const double thr = u * tot;
              double acc = 0.0;
              bool hit = false;
              for (int r = b.x0; r < b.x1 && !hit; ++r) {
                acc += rw[rowwin_index(r, y, H)];
                hit = u > 0.0 && bits(acc) == bits(thr);
              }
              exact += hit;
              const bool inside = bx >= b.x0 && bx < b.x1 && by >= b.y0 && by < b.y1;
              if (ax != bx || ay != by || !inside) {
                ++mismatches;
                fprintf(stderr, "draw %dx%d kind %d md %d at (%d,%d) u=%.17g: (%d,%d) without the table, (%d,%d) with it\n", H, W,
                        kind, md, x, y, u, ax, ay, bx, by);
              }
            }
          }
      }
  printf("maps=%ld draws=%ld segs=%ld over17=%ld exact=%ld mismatches=%ld\n", maps, draws, segs, over17, exact, mismatches);
  return mismatches ? 1 : 0;
}
