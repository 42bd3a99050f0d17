// select_plan.h - how select.hip lays a selection of the resident patterns on the chip: pure functions of the element
// size, the detector shape, the rectangle with its steps and the number of output patterns, no HIP call
// (tests/test_host_select.py compiles this header with the host compiler and checks the choice over the cases of the GPU
// table).
//
//   out[i, r, c] = in[index[i], row0 + r * row_step, col0 + c * col_step],   r < n_rows, c < n_cols
//
// The copy is byte-exact and memory-bound.  What decides the path is how long the contiguous runs of source bytes are:
//   path 0 (whole):   full-width rows one after the other (col0 = 0, n_cols = sx, row_step = 1; the whole detector is
//                     the common case): ONE run of n_rows * sx * esize bytes per pattern.
//   path 1 (rows):    col_step = 1: a run of n_cols * esize bytes per output row.
//   path 2 (strided): col_step > 1: no two wanted elements touch; one element per lane.
// Paths 0 and 1 share a kernel.  A lane owns one 16-byte piece of the OUTPUT, aligned to 16 bytes in the destination
// buffer, so every full piece is one 16-byte store; the pieces at the two ends of a pattern's output and those that
// straddle two runs are written byte by byte by the same lane, each byte once.  `items` is the most such pieces an
// output pattern can touch, whatever its start's alignment.  Small outputs share a workgroup (`patterns_per_block`, at
// most SEL_MAX_PATTERNS_PER_BLOCK - a cap that binds only for outputs of under 48 bytes, whose launch is tiny either way;
// it makes 65 the first pattern count that needs a second workgroup whatever the shape, which the tests reach); large
// ones take several (`grid_x`); `grid_y` walks the pattern groups, looping when there are more than the grid holds.
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int SEL_THREADS = 256;
constexpr int SEL_PIECE = 16;                      // bytes a lane moves at once on paths 0 and 1
constexpr int SEL_MAX_PATTERNS_PER_BLOCK = 64;     // of small outputs that share a workgroup
constexpr int64_t SEL_MAX_GRID_Y = 65535;
constexpr int64_t SEL_MAX_PATTERN_BYTES = (int64_t)1 << 31;  // offsets inside ONE pattern are 32-bit, all others int64

enum { SEL_WHOLE = 0, SEL_ROWS = 1, SEL_STRIDED = 2 };

struct SelPlan {
  int path;                  // SEL_*, -1: the arguments are not a selection of an sy x sx detector
  int esize;                 // bytes per element
  unsigned run_bytes;        // paths 0 / 1: contiguous source bytes per run
  unsigned runs;             // paths 0 / 1: runs per output pattern (1 / n_rows)
  unsigned out_bytes;        // bytes of one output pattern
  unsigned items;            // lane items per output pattern: 16-byte pieces (paths 0 / 1), elements (path 2)
  unsigned patterns_per_block;  // output patterns that share a workgroup (items <= SEL_THREADS / 2), else 1
  unsigned grid_x, grid_y;   // grid_x workgroups cover the items of one group of patterns_per_block patterns
};

// does [first, first + (n - 1) * step] lie inside [0, size)?
inline bool sel_range_ok(int first, int step, int n, int size) {
  return first >= 0 && step >= 1 && n >= 1 && first < size && (int64_t)first + (int64_t)(n - 1) * step < (int64_t)size;
}

inline SelPlan select_plan(int esize, int sy, int sx, int64_t n_out, int row0, int row_step, int n_rows, int col0, int col_step,
                           int n_cols) {
  SelPlan p{};
  p.path = -1;
  if ((esize != 1 && esize != 2 && esize != 4 && esize != 8) || sy < 1 || sx < 1 || n_out < 1 ||
      !sel_range_ok(row0, row_step, n_rows, sy) || !sel_range_ok(col0, col_step, n_cols, sx) ||
      (int64_t)sy * sx * esize >= SEL_MAX_PATTERN_BYTES)
    return p;
  p.esize = esize;
  p.out_bytes = (unsigned)((int64_t)n_rows * n_cols * esize);
  if (col_step > 1 && n_cols > 1) {
    p.path = SEL_STRIDED;
    p.items = (unsigned)(n_rows * (int64_t)n_cols);
  } else {
    // (a single column is a run of one element whatever its step)
    const bool whole = n_cols == sx && (row_step == 1 || n_rows == 1);
    p.path = whole ? SEL_WHOLE : SEL_ROWS;
    p.runs = whole ? 1u : (unsigned)n_rows;
    p.run_bytes = p.out_bytes / p.runs;
    // a pattern's output starts anywhere in its first piece: at most this many pieces hold a byte of it
    p.items = (p.out_bytes + (SEL_PIECE - 1) + (SEL_PIECE - 1)) / SEL_PIECE;
  }
  p.patterns_per_block = p.items <= (unsigned)SEL_THREADS / 2 ? (unsigned)SEL_THREADS / p.items : 1u;
  if (p.patterns_per_block > (unsigned)SEL_MAX_PATTERNS_PER_BLOCK) p.patterns_per_block = SEL_MAX_PATTERNS_PER_BLOCK;
  p.grid_x = p.patterns_per_block > 1 ? 1u : (p.items + SEL_THREADS - 1) / SEL_THREADS;
  const int64_t groups = (n_out + p.patterns_per_block - 1) / p.patterns_per_block;
  p.grid_y = (unsigned)(groups < SEL_MAX_GRID_Y ? groups : SEL_MAX_GRID_Y);
  return p;
}

}  // namespace kpdi
