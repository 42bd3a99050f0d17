// fftfilter_plan.h - how fftfilter.hip lays the FFT filter of a pattern set on the chip: pure functions of the domain, the
// detector shape and the number of patterns, no HIP call (tests/test_host_fft_filter.py compiles this header with the
// host compiler and checks the choice over a sweep of shapes).
//
//   path 0 (LDS):       one workgroup per pattern, one kernel, one pass over HBM.  Frequency domain: the pattern (f32)
//                       and two sy x (sx/2 + 1) complex intermediates of the half-spectrum DFT, plus both twiddle
//                       tables, stay in LDS.  Spatial domain: the pattern (f32) and the filtered pattern (f32).
//   path 1 (workspace): the intermediates go to a device workspace; a few kernels per batch of patterns, each spread
//                       over many workgroups per pattern (frequency: statistics, row DFT, column DFT x table, inverse
//                       column DFT, inverse row DFT, epilogue; spatial: statistics, correlation, epilogue).  A batch
//                       holds as many patterns as PATTERN_WORKSPACE_CAP admits (1024 x 1024 in the frequency domain needs
//                       8.4 MB per pattern).
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int FF_THREADS = 256;
constexpr int FF_DOMAIN_FREQUENCY = 0, FF_DOMAIN_SPATIAL = 1;  // = KPDI_DOMAIN_FREQUENCY / KPDI_DOMAIN_SPATIAL
constexpr size_t FF_RED_BYTES = 4 * (FF_THREADS / 64) * 8;   // block reductions: 4 doubles per wave

struct FfPlan : PatternPath {
  int blocks_half;  // path 1: workgroups per pattern over the sy x (sx/2 + 1) half spectrum
  int blocks_pix;   // path 1: workgroups per pattern over the sy x sx pixels
};

inline size_t ff_pix4(int sy, int sx) { return ((size_t)sy * sx + 3) & ~(size_t)3; }

// path 0, frequency: pattern / result (f32, padded to quads) + two intermediates (float2) + twiddles (float2) + reduction
// path 0, spatial:   pattern (f32) + result (f32) + reduction
inline size_t ff_lds_path_bytes(int domain, int sy, int sx) {
  if (domain == FF_DOMAIN_SPATIAL) return 2 * ff_pix4(sy, sx) * 4 + FF_RED_BYTES;
  const size_t inter = (size_t)sy * half_cols(sx);
  return ff_pix4(sy, sx) * 4 + 2 * inter * 8 + ((size_t)sx + sy) * 8 + FF_RED_BYTES;
}

// path 1, per pattern: frequency: X and G (float2 each; the f32 result reuses G), spatial: the f32 result; both: the
// statistics (2 doubles: mean, non-finite)
inline size_t ff_ws_pattern_bytes(int domain, int sy, int sx) {
  if (domain == FF_DOMAIN_SPATIAL) return ff_pix4(sy, sx) * 4 + 2 * 8;
  return 2 * (size_t)sy * half_cols(sx) * 8 + 2 * 8;
}

// path 1 LDS: the twiddles of the longer axis + the reduction
inline size_t ff_ws_lds_bytes(int sy, int sx) { return (size_t)(sx > sy ? sx : sy) * 8 + FF_RED_BYTES; }

// `n` patterns of sy x sx.  `force_workspace`: path 1 for a shape path 0 takes (tests: KPDI_FFT_FILTER_PATH=1);
// `max_batch` > 0: a cap on the patterns per batch of path 1 (tests: KPDI_PATTERN_BATCH)
inline FfPlan ff_plan(int domain, int sy, int sx, int64_t n, bool force_workspace = false, int64_t max_batch = 0) {
  if (sy < 1 || sx < 1 || n < 1 || (domain != FF_DOMAIN_FREQUENCY && domain != FF_DOMAIN_SPATIAL)) return FfPlan{{-1}};
  FfPlan p{pattern_path(ff_lds_path_bytes(domain, sy, sx), ff_ws_lds_bytes(sy, sx), ff_ws_pattern_bytes(domain, sy, sx), n,
                        force_workspace, max_batch)};
  if (p.path == 1) {
    const size_t inter = (size_t)sy * half_cols(sx), npix = (size_t)sy * sx;
    p.blocks_half = (int)((inter + FF_THREADS - 1) / FF_THREADS);
    p.blocks_pix = (int)((npix + FF_THREADS - 1) / FF_THREADS);
  }
  return p;
}

}  // namespace kpdi
