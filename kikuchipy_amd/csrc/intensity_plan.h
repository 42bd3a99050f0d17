// intensity_plan.h - how intensity.hip lays intensity rescaling / normalization of a pattern set on the chip: pure
// functions of the dtype, the detector shape and the number of patterns, no HIP call (tests/test_host_intensity.py
// compiles this header with the host compiler and checks the choice over a sweep of shapes).
//
//   path 0 (LDS):   one workgroup per pattern; the pattern is copied into LDS once (16-byte loads where the pattern
//                   allows them), and every pass of the call (min / max, the radix-select passes of percentiles, mean
//                   and standard deviation, the map and the cast) reads it from there: one read of HBM, one write.
//   path 1 (L2):    one workgroup per pattern, every pass re-reads the pattern from L2 / HBM; for patterns whose bytes
//                   exceed INT_LDS_CAP (up to 1024 x 1024 float64 and beyond).
// Both paths visit the pixels in the same order (thread t takes the quads t, t + INT_THREADS, ...), so their
// reductions, and so their results, are bit-identical.
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int INT_THREADS = 256;                // 4 waves: one per order statistic in the radix select
constexpr size_t INT_LDS_CAP = 64 * 1024;       // the staged pattern; with the histograms ~70 KiB: two workgroups / CU
constexpr int INT_RANGE_BLOCKS = 1024;          // kpdi_intensity_range: partial min / max per block, then one block
constexpr int INT_MODE_MINMAX = 0, INT_MODE_RANGE = 1, INT_MODE_PERCENTILE = 2, INT_MODE_NORMALIZE = 3;

struct IntPlan {
  int path;          // 0 LDS, 1 L2, -1 no path takes the shape / dtype
  size_t lds_bytes;  // dynamic LDS per workgroup (the staged pattern)
  int select_passes; // radix-select passes of 8 bits for percentiles: 1 (8-bit), 2 (16-bit), 4 (f32), 8 (f64)
};

inline size_t int_staged_bytes(int dtype, int sy, int sx) {
  return ((size_t)sy * sx * pattern_dtype_bytes(dtype) + 15) & ~(size_t)15;
}

inline IntPlan int_plan(int dtype, int sy, int sx, int64_t n) {
  IntPlan p{};
  const int es = pattern_dtype_bytes(dtype);
  if (sy < 1 || sx < 1 || n < 1 || es == 0 || (int64_t)sy * sx >= ((int64_t)1 << 30) || n >= (int64_t)INT32_MAX) {
    p.path = -1;
    return p;
  }
  p.select_passes = es;
  const size_t staged = int_staged_bytes(dtype, sy, sx);
  if (staged <= INT_LDS_CAP) {
    p.path = 0;
    p.lds_bytes = staged;
  } else {
    p.path = 1;
    p.lds_bytes = 0;
  }
  return p;
}

}  // namespace kpdi
