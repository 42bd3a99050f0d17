// iq_plan.h - how iq.hip lays the image quality of a pattern set on the chip: pure functions of the detector shape and
// the number of patterns, no HIP call (tests/test_host_image_quality.py compiles this header with the host compiler and
// checks the choice over a sweep of shapes).
//
//   path 0 (LDS):       one workgroup per pattern; the pattern (f32), both twiddle tables and the sy x (sx/2 + 1)
//                       complex intermediate of the half-spectrum DFT stay in LDS - one kernel, one pass over HBM.
//   path 1 (workspace): the intermediate goes to a device workspace; four kernels per batch of patterns (statistics,
//                       row DFT, column DFT + partial sums, final sums), each spread over many workgroups per pattern.
//                       A batch holds as many patterns as IQ_WORKSPACE_CAP admits (at least one: 1024 x 1024 needs 4.2 MB).
#pragma once
#include <cstddef>
#include <cstdint>

namespace kpdi {

constexpr int IQ_THREADS = 256;
constexpr size_t IQ_LDS_CAP = 150 * 1024;           // of the 160 KiB per CU, as the fused pre-processing kernel
constexpr size_t IQ_WORKSPACE_CAP = (size_t)256 << 20;  // path 1: intermediates + partial sums of one batch

struct IqPlan {
  int path;                // 0 LDS, 1 workspace
  size_t lds_bytes;        // dynamic LDS per workgroup
  int64_t batch;           // path 1: patterns per batch of launches
  int blocks_per_pattern;  // path 1: workgroups per pattern of the row and column kernels
  size_t workspace_bytes;  // path 1: what one batch needs (<= IQ_WORKSPACE_CAP)
};

inline int iq_half_cols(int sx) { return sx / 2 + 1; }

// path 0: pattern (f32) + intermediate (float2) + twiddles for sx and sy (float2) + the block reduction (4 doubles per wave)
inline size_t iq_lds_path_bytes(int sy, int sx) {
  const size_t npix = (size_t)sy * sx, inter = (size_t)sy * iq_half_cols(sx);
  return ((npix + 1) & ~(size_t)1) * 4 + inter * 8 + ((size_t)sx + sy) * 8 + 4 * (IQ_THREADS / 64) * 8;
}

// path 1: twiddles + reduction only
inline size_t iq_ws_lds_bytes(int sy, int sx) { return ((size_t)sx + sy) * 8 + 4 * (IQ_THREADS / 64) * 8; }

// per pattern in path 1: the intermediate, the statistics (3 doubles) and 2 partial sums per column-kernel workgroup
inline size_t iq_ws_pattern_bytes(int sy, int sx) {
  const size_t inter = (size_t)sy * iq_half_cols(sx);
  const size_t blocks = (inter + IQ_THREADS - 1) / IQ_THREADS;
  return inter * 8 + 3 * 8 + blocks * 2 * 8;
}

// `n` patterns of sy x sx; path = -1 when no path can take the shape
inline IqPlan iq_plan(int sy, int sx, int64_t n) {
  IqPlan p{};
  if (sy < 1 || sx < 1 || n < 1) {
    p.path = -1;
    return p;
  }
  const size_t lds = iq_lds_path_bytes(sy, sx);
  if (lds <= IQ_LDS_CAP) {
    p.path = 0;
    p.lds_bytes = lds;
    p.batch = n;
    return p;
  }
  const size_t per = iq_ws_pattern_bytes(sy, sx);
  p.lds_bytes = iq_ws_lds_bytes(sy, sx);
  if (per > IQ_WORKSPACE_CAP || p.lds_bytes > IQ_LDS_CAP) {
    p.path = -1;
    return p;
  }
  p.path = 1;
  const int64_t fit = (int64_t)(IQ_WORKSPACE_CAP / per);
  p.batch = n < fit ? n : fit;
  const size_t inter = (size_t)sy * iq_half_cols(sx);
  p.blocks_per_pattern = (int)((inter + IQ_THREADS - 1) / IQ_THREADS);
  p.workspace_bytes = (size_t)p.batch * per;
  return p;
}

}  // namespace kpdi
