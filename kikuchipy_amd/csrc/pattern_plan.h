// pattern_plan.h - what the plans of the per-pattern pre-processing ops (iq_plan.h, fftfilter_plan.h, intensity_plan.h,
// clahe_plan.h) share: the LDS and workspace caps, the half-spectrum width, the element size of the pattern dtypes and
// the choice between one workgroup per pattern in LDS and batches of a device workspace.  Pure functions, no HIP call:
// the tests compile these headers with the host compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/kpdi.h"

// helpers that the kernels evaluate too
#if defined(__HIPCC__) || defined(__HIP__)
#define PLAN_HD __host__ __device__
#else
#define PLAN_HD
#endif

namespace kpdi {

constexpr size_t PATTERN_LDS_CAP = 150 * 1024;                // of the 160 KiB per CU, as the fused pre-processing kernel
constexpr size_t PATTERN_WORKSPACE_CAP = (size_t)256 << 20;  // path 1: intermediates + statistics of one batch

// columns l = 0 ... sx/2 of the half spectrum of a real pattern
PLAN_HD inline int half_cols(int sx) { return sx / 2 + 1; }

// bytes of an element of the six pattern dtypes (KPDI_U8, I8, U16, I16, F32, F64), 0 for any other dtype
inline int pattern_dtype_bytes(int dtype) {
  switch (dtype) {
    case KPDI_U8: case KPDI_I8: return 1;
    case KPDI_U16: case KPDI_I16: return 2;
    case KPDI_F32: return 4;
    case KPDI_F64: return 8;
    default: return 0;
  }
}

struct PatternPath {
  int path;                // 0 LDS, 1 workspace, -1 no path takes the shape
  size_t lds_bytes;        // dynamic LDS per workgroup
  int64_t batch;           // patterns per batch of launches
  size_t workspace_bytes;  // path 1: what one batch needs (<= PATTERN_WORKSPACE_CAP)
};

// `n` patterns: path 0 when its `lds` bytes fit, else path 1 (`ws_lds` bytes of LDS, `per` bytes of workspace per
// pattern) in batches of as many patterns as PATTERN_WORKSPACE_CAP admits.  `force_workspace`: path 1 for a shape that
// path 0 would take; `max_batch` > 0: at most that many patterns per batch (`workspace_bytes` follows).  Both are for
// the tests, which reach the workspace path and a second batch at small shapes with them.
inline PatternPath pattern_path(size_t lds, size_t ws_lds, size_t per, int64_t n, bool force_workspace = false,
                                int64_t max_batch = 0) {
  PatternPath p{};
  if (lds <= PATTERN_LDS_CAP && !force_workspace) {
    p.path = 0;
    p.lds_bytes = lds;
    p.batch = n;
    return p;
  }
  p.lds_bytes = ws_lds;
  if (per > PATTERN_WORKSPACE_CAP || ws_lds > PATTERN_LDS_CAP) {
    p.path = -1;
    return p;
  }
  p.path = 1;
  const int64_t fit = (int64_t)(PATTERN_WORKSPACE_CAP / per);
  p.batch = n < fit ? n : fit;
  if (max_batch > 0 && p.batch > max_batch) p.batch = max_batch;
  p.workspace_bytes = (size_t)p.batch * per;
  return p;
}

}  // namespace kpdi
