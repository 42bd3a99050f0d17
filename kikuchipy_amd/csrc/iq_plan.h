// iq_plan.h - how iq.hip lays the image quality of a pattern set on the chip: pure functions of the detector shape and
// the number of patterns, no HIP call (tests/test_host_image_quality.py compiles this header with the host compiler and
// checks the choice over a sweep of shapes).
//
//   path 0 (LDS):       one workgroup per pattern; the pattern (f32), both twiddle tables and the sy x (sx/2 + 1)
//                       complex intermediate of the half-spectrum DFT stay in LDS - one kernel, one pass over HBM.
//   path 1 (workspace): the intermediate goes to a device workspace; four kernels per batch of patterns (statistics,
//                       row DFT, column DFT + partial sums, final sums), each spread over many workgroups per pattern.
//                       A batch holds as many patterns as PATTERN_WORKSPACE_CAP admits (at least one: 1024 x 1024 needs 4.2 MB).
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int IQ_THREADS = 256;

struct IqPlan : PatternPath {
  int blocks_per_pattern;  // path 1: workgroups per pattern of the row and column kernels
};

// path 0: pattern (f32) + intermediate (float2) + twiddles for sx and sy (float2) + the block reduction (4 doubles per wave)
inline size_t iq_lds_path_bytes(int sy, int sx) {
  const size_t npix = (size_t)sy * sx, inter = (size_t)sy * half_cols(sx);
  return ((npix + 1) & ~(size_t)1) * 4 + inter * 8 + ((size_t)sx + sy) * 8 + 4 * (IQ_THREADS / 64) * 8;
}

// path 1: twiddles + reduction only
inline size_t iq_ws_lds_bytes(int sy, int sx) { return ((size_t)sx + sy) * 8 + 4 * (IQ_THREADS / 64) * 8; }

// per pattern in path 1: the intermediate, the statistics (3 doubles) and 2 partial sums per column-kernel workgroup
inline size_t iq_ws_pattern_bytes(int sy, int sx) {
  const size_t inter = (size_t)sy * half_cols(sx);
  const size_t blocks = (inter + IQ_THREADS - 1) / IQ_THREADS;
  return inter * 8 + 3 * 8 + blocks * 2 * 8;
}

// `n` patterns of sy x sx; path = -1 when no path can take the shape.  `force_workspace`: path 1 for a shape path 0
// takes (tests: KPDI_IQ_PATH=1); `max_batch` > 0: a cap on the patterns per batch of path 1 (tests: KPDI_PATTERN_BATCH)
inline IqPlan iq_plan(int sy, int sx, int64_t n, bool force_workspace = false, int64_t max_batch = 0) {
  if (sy < 1 || sx < 1 || n < 1) return IqPlan{{-1}};
  IqPlan p{pattern_path(iq_lds_path_bytes(sy, sx), iq_ws_lds_bytes(sy, sx), iq_ws_pattern_bytes(sy, sx), n, force_workspace,
                        max_batch)};
  if (p.path == 1) p.blocks_per_pattern = (int)(((size_t)sy * half_cols(sx) + IQ_THREADS - 1) / IQ_THREADS);
  return p;
}

}  // namespace kpdi
