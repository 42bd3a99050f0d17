// clahe_plan.h - how clahe.hip lays adaptive histogram equalization (CLAHE) of a pattern set on the chip: pure functions
// of the dtype, the detector shape, the kernel (contextual region) shape, the number of bins and the number of
// patterns, no HIP call (tests/test_host_clahe.py compiles this header with the host compiler and checks the choice
// over a sweep of shapes, kernels and bin counts).
//
// One workgroup takes one pattern.  The padded image is tiled by the kernel: nty x ntx = ceil(sy / ky) x ceil(sx / kx)
// tile histograms of `nbins` bins, one uint16 lookup table per tile, and (nty + 1) x (ntx + 1) interpolation blocks.
//   path 0 (LDS):       the pattern's bins, every tile histogram and table, and the row / column tables (see
//                       clahe_table_bytes) live in LDS (CLAHE_LDS_CAP); histograms use LDS atomics.
//   path 1 (workspace): the pattern's bins and its 14-bit result in a global workspace slot, the histograms and tables
//                       of a band of `band` tile rows (plus the previous row's tables) there too, band after band; the
//                       histograms use global (vector) atomics; the row / column tables stay in LDS.  Patterns run in launches of `per_launch` so that the
//                       workspace stays under CLAHE_WS_CAP; beyond it there is no path.
// Both paths do the same integer work per tile and the same per-pixel arithmetic, so they give the same bits.
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int CLAHE_THREADS = 256;
constexpr size_t CLAHE_LDS_CAP = 64 * 1024;           // path 0: ~21 KiB at 60 x 60, kernel 15 x 15, 128 bins
constexpr size_t CLAHE_WS_CAP = (size_t)512 << 20;    // path 1: the whole workspace
constexpr size_t CLAHE_WS_BAND_BYTES = (size_t)16 << 20;  // path 1: a band's histograms + tables per pattern, target
constexpr size_t CLAHE_TABLE_CAP = 128 * 1024;        // path 1's LDS: the row / column tables
constexpr int CLAHE_MAX_NBINS = 16384;                // 2**14 grey levels: more bins than levels is refused
constexpr int CLAHE_WS_MAX_PER_LAUNCH = 4096;

struct ClahePlan {
  int path;             // 0 LDS, 1 workspace, -1 no path takes the shape / kernel / bins
  int nty, ntx;         // tile histograms per axis: ceil(sy / ky), ceil(sx / kx)
  int band;             // tile rows per band (path 0: all of them)
  size_t lds_bytes;     // dynamic LDS per workgroup
  size_t slot_bytes;    // path 1: workspace per pattern
  int64_t per_launch;   // path 1: patterns per launch
  size_t workspace_bytes;  // path 1: slot_bytes * per_launch
};

PLAN_HD inline size_t clahe_align(size_t b) { return (b + 15) & ~(size_t)15; }

// the LDS tables both paths keep: per detector row / column its interpolation block (int) and weight offset / k
// (double); per row / column of the histogrammed region (nty * ky x ntx * kx, reflected past the pattern's end) the
// detector row / column it reads and its tile (2 ints)
PLAN_HD inline size_t clahe_table_bytes(int sy, int sx, int nty, int ntx, int ky, int kx) {
  return clahe_align(((size_t)sy + sx) * (sizeof(int) + sizeof(double))) +
         clahe_align(((size_t)nty * ky + (size_t)ntx * kx) * 2 * sizeof(int));
}

// LDS layout of path 0: bins / result (uint16, npix), histograms (uint32), tables (uint16), then the row / column tables
inline size_t clahe_lds_bytes(int sy, int sx, int nty, int ntx, int nbins, int ky, int kx) {
  const size_t nt = (size_t)nty * ntx;
  return clahe_align((size_t)sy * sx * 2) + clahe_align(nt * nbins * 4) + clahe_align(nt * nbins * 2) +
         clahe_table_bytes(sy, sx, nty, ntx, ky, kx);
}

// workspace slot of path 1: bins (uint16), result (uint16), the band's histograms (uint32), band + 1 rows of tables
inline size_t clahe_slot_bytes(int sy, int sx, int ntx, int nbins, int band) {
  const size_t row = (size_t)ntx * nbins;
  return clahe_align((size_t)sy * sx * 2) * 2 + clahe_align(row * band * 4) + clahe_align(row * (band + 1) * 2);
}

// path 1's band, slot and launch size; `split`: at most half the tile rows per band (so that the band loop runs more
// than once wherever there are two tile rows or more)
inline bool clahe_fill_workspace(ClahePlan &p, int sy, int sx, int ky, int kx, int nbins, int64_t n, bool split) {
  const size_t row = (size_t)p.ntx * nbins * 6;  // histograms + tables of one tile row
  int64_t band = (int64_t)(CLAHE_WS_BAND_BYTES / row);
  if (band < 1) band = 1;
  if (band > p.nty) band = p.nty;
  if (split && band > 1 && band >= p.nty) band = (p.nty + 1) / 2;
  p.band = (int)band;
  p.slot_bytes = clahe_slot_bytes(sy, sx, p.ntx, nbins, p.band);
  if (p.slot_bytes > CLAHE_WS_CAP) {
    p.band = 1;
    p.slot_bytes = clahe_slot_bytes(sy, sx, p.ntx, nbins, 1);
    if (p.slot_bytes > CLAHE_WS_CAP) return false;
  }
  int64_t per = (int64_t)(CLAHE_WS_CAP / p.slot_bytes);
  if (per > CLAHE_WS_MAX_PER_LAUNCH) per = CLAHE_WS_MAX_PER_LAUNCH;
  if (per > n) per = n;
  p.path = 1;
  p.lds_bytes = clahe_table_bytes(sy, sx, p.nty, p.ntx, ky, kx);
  p.per_launch = per;
  p.workspace_bytes = p.slot_bytes * (size_t)per;
  return true;
}

// `force_workspace`: path 1 for a shape path 0 takes (tests: KPDI_CLAHE_PATH=1)
inline ClahePlan clahe_plan(int dtype, int sy, int sx, int ky, int kx, int nbins, int64_t n,
                            bool force_workspace = false) {
  ClahePlan p{};
  p.path = -1;
  if (sy < 1 || sx < 1 || ky < 1 || kx < 1 || nbins < 1 || nbins > CLAHE_MAX_NBINS || n < 1 ||
      n >= (int64_t)INT32_MAX || pattern_dtype_bytes(dtype) == 0)
    return p;
  if ((int64_t)sy * sx >= ((int64_t)1 << 30) || (int64_t)ky * kx >= ((int64_t)1 << 30) || ky >= (1 << 20) ||
      kx >= (1 << 20))
    return p;
  p.nty = (int)((sy + (int64_t)ky - 1) / ky);
  p.ntx = (int)((sx + (int64_t)kx - 1) / kx);
  if (clahe_table_bytes(sy, sx, p.nty, p.ntx, ky, kx) > CLAHE_TABLE_CAP) return p;
  const size_t lds = clahe_lds_bytes(sy, sx, p.nty, p.ntx, nbins, ky, kx);
  if (lds <= CLAHE_LDS_CAP && !force_workspace) {
    p.path = 0;
    p.band = p.nty;
    p.lds_bytes = lds;
    return p;
  }
  if (!clahe_fill_workspace(p, sy, sx, ky, kx, nbins, n, lds <= CLAHE_LDS_CAP)) p.path = -1;
  return p;
}

}  // namespace kpdi
