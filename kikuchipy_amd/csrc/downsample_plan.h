// downsample_plan.h - how downsample.hip lays the binning of a pattern set on the chip: pure functions of the dtype, the
// detector shape, the factor and the number of patterns, no HIP call (tests/test_host_downsample.py compiles this header
// with the host compiler and checks the choice over a sweep of shapes).
//
// One workgroup per pattern: a single wave for small binned images (DS_WAVE_PIXELS; 60 x 60 -> 30 x 30), else four.  A
// lane owns binned pixels o, o + threads, ... and adds each one's factor x factor source pixels in the reference's
// order, so the sums do not depend on the path, the workgroup size or anything else chosen here.
//   path 0 (LDS):       the binned float32 image lives in LDS between the binning pass, the min / max reduction and the
//                       rescale-and-store pass (480 x 480 -> 120 x 120: 57.6 KB).  `staged`: the raw pattern fits beside
//                       it and is brought in with 16-byte loads first (60 x 60 uint8: 3.6 KB + 3.6 KB).
//   path 1 (workspace): binned images that do not fit (2048 x 2048 at factor 2: 4 MB) go to a device workspace, one
//                       slot per workgroup; `grid` persistent workgroups walk the patterns.
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int DS_THREADS = 256;
constexpr int DS_WAVE_PIXELS = 1024;          // binned images of up to this many pixels take one wave
constexpr size_t DS_LDS_CAP = 60 * 1024;      // dynamic LDS of a workgroup: two of them and their statics per CU
constexpr int DS_MAX_GRID = 1024;             // path 1: persistent workgroups

struct DsPlan : PatternPath {
  int threads;       // 64 or DS_THREADS
  int staged;        // path 0: the raw pattern is copied into LDS first
  size_t raw_bytes;  // staged: its bytes rounded up to 16; the binned image follows them
  int grid;          // workgroups (path 0: one per pattern)
};

// `force_workspace`: path 1 for a shape that path 0 would take (the tests compare the two)
inline DsPlan ds_plan(int dtype, int sy, int sx, int factor, int64_t n, bool force_workspace = false) {
  DsPlan p{};
  p.path = -1;
  const size_t es = (size_t)pattern_dtype_bytes(dtype);
  if (!es || factor < 2 || sy < factor || sx < factor || sy % factor || sx % factor || n < 1 || n >= (int64_t)INT32_MAX ||
      (int64_t)sy * sx >= ((int64_t)1 << 30))
    return p;
  const size_t nout = (size_t)(sy / factor) * (size_t)(sx / factor), binned = nout * sizeof(float);
  p.threads = nout <= (size_t)DS_WAVE_PIXELS ? 64 : DS_THREADS;
  p.batch = n;
  if (!force_workspace && binned <= DS_LDS_CAP) {
    p.path = 0;
    const size_t raw = ((size_t)sy * sx * es + 15) & ~(size_t)15;
    p.staged = raw + binned <= DS_LDS_CAP;
    p.raw_bytes = p.staged ? raw : 0;
    p.lds_bytes = p.raw_bytes + binned;
    p.grid = (int)n;
    return p;
  }
  if (binned > PATTERN_WORKSPACE_CAP) return p;
  const int64_t fit = (int64_t)(PATTERN_WORKSPACE_CAP / binned);
  int64_t g = n < DS_MAX_GRID ? n : DS_MAX_GRID;
  if (g > fit) g = fit;
  p.path = 1;
  p.grid = (int)g;
  p.workspace_bytes = (size_t)g * binned;
  return p;
}

}  // namespace kpdi
