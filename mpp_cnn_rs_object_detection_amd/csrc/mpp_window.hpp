// mpp_window.hpp -- the window of the data-driven translation (transform_kernels.py:70-99): its bounds, the sum of one of
// its rows, the transposed table of those sums (rowwin) and the draw of a pixel in the form one lane runs on its own.
// Nothing of the chain is needed here: the kernels that build the tables (mpp_maps.hip), the draws (mpp_chain.hpp) and a
// stand-alone host program (tests/window_walk.hip) take the arithmetic from this one place.
//
// rowwin[y * H + x] is the sum of det over row x of the window around any pixel of column y: the window's columns
// [y0, y1) depend on y alone.  A draw at (x, y) walks rows x0 .. x1 - 1 of column y's window -- consecutive entries of the
// table, where the per-row prefix table rowpart has two entries per row in rows that lie W * 8 bytes apart.  An entry is
// window_row_seg() of the same two doubles, so a draw that reads the table adds up the bits a draw without it forms.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

#define MPP_WIN_ROWS 17        // rows (and columns) of the window the unrolled form of window_draw_rows() takes: max_delta <= 8
// The unrolled form reads MPP_WIN_ROWS consecutive entries from the window's first row on, whatever the number of rows
// the tile leaves the window: the entries behind the last row (of the next column, of the next tile's table, or of this
// pad behind the last table) are read and never used.
#define MPP_ROWWIN_PAD (MPP_WIN_ROWS - 1)

// (the diagnostic build of the deep rounds, MPP_DEEP_PROF in mpp_deep.hip, defines these two to clock the draw at three
//  points: the window's total, the row and the column known; everywhere else they are nothing)
#ifndef MPP_WIN_STAMP
#define MPP_WIN_T0()
#define MPP_WIN_STAMP(i, v)
#endif

struct WinBox { int x0, x1, y0, y1; };      // rows [x0, x1), columns [y0, y1): the (2 * md + 1)^2 window clipped to the tile
__host__ __device__ __forceinline__ WinBox window_box(int x, int y, int md, int H, int W) {
  WinBox b;
  b.x0 = x - md > 0 ? x - md : 0; b.x1 = x + md + 1 < H ? x + md + 1 : H;
  b.y0 = y - md > 0 ? y - md : 0; b.y1 = y + md + 1 < W ? y + md + 1 : W;
  return b;
}
__host__ __device__ __forceinline__ size_t rowwin_index(int x, int y, int H) { return (size_t)y * H + x; }
// doubles of the tables of n_maps tiles, one behind the other, and the pad
__host__ __device__ __forceinline__ size_t rowwin_count(size_t n_maps, int H, int W) {
  return n_maps * (size_t)H * W + MPP_ROWWIN_PAD;
}
// sum of det over columns [y0, y1) of the row whose inclusive prefix sums are rp[]
template <typename DP>
__host__ __device__ __forceinline__ double window_row_seg(DP rp, int y0, int y1) {
  return rp[y1 - 1] - (y0 > 0 ? rp[y0 - 1] : 0.0);
}

// The draw, one lane on its own: a pixel of the window around (x, y) with probability det / boxsum.  The row is found by
// adding the rows' sums top to bottom while the partial sum stays <= u * tot, the column by counting the prefix sums of
// that row that do.  rowwin == nullptr: the rows' sums are formed from rowpart.  DP: pointer to const double (the kernels
// pass pointers into global memory).
template <typename DP>
__host__ __device__ __forceinline__ void window_draw_rows(DP rowpart, DP boxsum, DP rowwin, int H, int W, int md, int x, int y,
                                                          double u, int *ex, int *ey) {
  MPP_WIN_T0();
  const WinBox b = window_box(x, y, md, H, W);
  const int x0 = b.x0, y0 = b.y0, y1 = b.y1;
  const int nrow = b.x1 - x0, wc = y1 - y0;
  const double tot = boxsum[(size_t)x * W + y];
  double before = 0.0;
  const double thr = u * tot;
  int row = 0;
  MPP_WIN_STAMP(0, tot);
  if (nrow <= MPP_WIN_ROWS && wc <= MPP_WIN_ROWS) {
    // the usual window (max_delta <= 8): the segment sums of all rows are requested together -- one memory latency for the
    // row with the table (17 entries in a row: two or three cache lines), two without it (34 cache lines), one for the
    // column, instead of two per row walked -- and added in the order of the walk below
    double seg[MPP_WIN_ROWS];
    if (rowwin) {
      DP rw = rowwin + rowwin_index(x0, y, H);
#pragma unroll
      for (int i = 0; i < MPP_WIN_ROWS; ++i) seg[i] = rw[i];
    } else {
#pragma unroll
      for (int i = 0; i < MPP_WIN_ROWS; ++i) {
        const int xi = x0 + (i < nrow ? i : nrow - 1);
        seg[i] = window_row_seg(rowpart + (size_t)xi * W, y0, y1);
      }
    }
    bool go = true;
#pragma unroll
    for (int i = 0; i < MPP_WIN_ROWS; ++i) {
      const double nxt = before + seg[i];
      go = go && i < nrow && nxt <= thr && i < nrow - 1;
      if (go) { before = nxt; row = i + 1; }
    }
    MPP_WIN_STAMP(1, row);
    DP rp = rowpart + (size_t)(x0 + row) * W;
    const double lead = y0 > 0 ? rp[y0 - 1] : 0.0;
    double cv[MPP_WIN_ROWS];
#pragma unroll
    for (int jj = 0; jj < MPP_WIN_ROWS; ++jj) cv[jj] = rp[y0 + (jj < wc ? jj : wc - 1)];
    int col = 0;
#pragma unroll
    for (int jj = 0; jj < MPP_WIN_ROWS; ++jj) col += (jj < wc && (before + (cv[jj] - lead)) <= thr) ? 1 : 0;
    if (col >= wc) col = wc - 1;
    MPP_WIN_STAMP(2, col);
    *ex = x0 + row; *ey = y0 + col;
    return;
  }
  for (int i = 0; i < nrow; ++i) {
    const double s = rowwin ? rowwin[rowwin_index(x0 + i, y, H)] : window_row_seg(rowpart + (size_t)(x0 + i) * W, y0, y1);
    const double nxt = before + s;
    if (nxt <= thr && i < nrow - 1) { before = nxt; row = i + 1; } else break;
  }
  DP rp = rowpart + (size_t)(x0 + row) * W;
  const double lead = y0 > 0 ? rp[y0 - 1] : 0.0;
  int col = 0;
  for (int jj = 0; jj < wc; ++jj) col += ((before + (rp[y0 + jj] - lead)) <= thr) ? 1 : 0;
  if (col >= wc) col = wc - 1;
  *ex = x0 + row; *ey = y0 + col;
}
