// regionsum_plan.h - how regionsum.hip lays the sums over detector rectangles on the chip: pure functions of the
// dtype, the detector shape and the numbers of patterns and rectangles, no HIP call (tests/test_host_vbse.py compiles
// this header with the host compiler).
//
// The unit of work is a block of whole pattern rows that one wave stages in LDS: as many rows as RS_BLOCK_BYTES hold.
//   path 0: the pattern is one block (60 x 60 uint8: 3.6 KB); the wave writes the pattern's sums.
//   path 1: several blocks per pattern (240 x 240 uint8: 8; 1024 x 1024 float64: one per row); every wave writes the
//           partial sums of its block to a device workspace and a second kernel adds them in block order.  Patterns go
//           in batches of as many as PATTERN_WORKSPACE_CAP admits.
// The blocks depend on dtype and shape alone, so the order of every sum does too: not on the number of patterns, the
// batch or the launch geometry.
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;   // blocks of rows per workgroup, a wave each
constexpr int RS_GROUP = 16;                // lanes that share a rectangle; 64 / RS_GROUP rectangles per pass of a wave
constexpr int RS_PIECE = 16;                // pixels of a row that a lane adds in one go
constexpr int RS_RECT_TILE = 256;           // rectangles whose bounds are in LDS at a time
constexpr size_t RS_BLOCK_BYTES = 8192;     // pattern bytes per wave: 4 waves x 5 workgroups stay within a CU's LDS

struct RsPlan : PatternPath {
  int rows_per_block;
  int blocks_per_pattern;
  size_t slot_bytes;  // LDS of one wave: its block, widened to the 16-byte chunks that hold it
};

// `n` patterns of sy x sx of `dtype`, `n_rects` rectangles; path = -1 when no path can take the shape
inline RsPlan rs_plan(int dtype, int sy, int sx, int64_t n, int n_rects) {
  RsPlan p{};
  p.path = -1;
  const size_t es = (size_t)pattern_dtype_bytes(dtype);
  if (!es || sy < 1 || sx < 1 || n < 1 || n_rects < 1 || (size_t)sx * es > RS_BLOCK_BYTES) return p;
  const size_t row = (size_t)sx * es;
  size_t rb = RS_BLOCK_BYTES / row;
  if (rb > (size_t)sy) rb = (size_t)sy;
  p.rows_per_block = (int)rb;
  p.blocks_per_pattern = (int)(((size_t)sy + rb - 1) / rb);
  p.slot_bytes = ((rb * row + 15) & ~(size_t)15) + 32;  // an unaligned block touches one chunk more at either end
  p.lds_bytes = (size_t)RS_RECT_TILE * 16 + RS_WAVES * p.slot_bytes;
  if (p.lds_bytes > PATTERN_LDS_CAP) return p;
  p.batch = n;
  if (p.blocks_per_pattern == 1) {
    p.path = 0;
    return p;
  }
  const size_t per = (size_t)p.blocks_per_pattern * (size_t)n_rects * 8;  // partial sums of one pattern
  if (per > PATTERN_WORKSPACE_CAP) return p;
  const int64_t fit = (int64_t)(PATTERN_WORKSPACE_CAP / per);
  p.path = 1;
  p.batch = n < fit ? n : fit;
  p.workspace_bytes = (size_t)p.batch * per;
  return p;
}

}  // namespace kpdi
