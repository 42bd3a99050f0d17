// reduce_plan.h - how reduce.hip lays a reduction of the resident patterns over a set of their four axes (ny, nx, sy, sx)
// on the chip: pure functions of the shape, the dtype, the op and the axis set, no HIP call (tests/test_host_reduce.py
// compiles this header with the host compiler).
//
// Axes of length 1 drop out and neighbouring axes that are both reduced or both kept merge.  What is left alternates,
// and every one of the 15 axis sets is the form
//     in[A][R1][M][R2][B]  ->  out[A][M][B]          (any of the five may be 1)
// with ONE reduced group in R2 and R1 = M = 1, or two of them around the kept M: (0, 2), (1, 3), (0, 3), (0, 1, 3) and
// (0, 2, 3).  The R = R1 * R2 reduced values of an output are numbered r = r1 * R2 + r2 and cut into slices of `slice`
// consecutive r.  A (slice, output) pair gives one partial; a second kernel combines the partials of an output: one lane
// in slice order, or - more than RED_COMBINE_SERIAL slices - RED_COMBINE_LANES lanes, lane g the slices g, g + 16, ... in
// that order, and the lanes then in lane order.
//   RED_COLS (B > 1, the inner axis survives): a lane owns `vec` consecutive outputs (16 bytes of a row of B) and walks
//     its slice of r; the rows of all A * M outputs are laid side by side over the lanes (red_cols_item), so short rows
//     fill a wave too.  A row's last, cut vector belongs to one lane, which reads its elements one by one.
//   RED_RUNS (B == 1, contiguous runs of R2 values are reduced): `group` lanes (a power of two, up to a wave) share an
//     output.  The part of every run inside the slice is cut into vectors of `vec` values from its first value on,
//     vector j belongs to lane j % group (red_runs_lane); the lanes are then combined by the xor butterfly group/2 ... 1.
// A slice is RED_COLS_SLICE rows (RED_COLS) or group * vec * RED_RUNS_VECS values (RED_RUNS), or the multiple of that
// which keeps the slices of one output at RED_MAX_SLICES or fewer.  The order in which the values of an output are combined follows from the shape,
// the dtype and the axis set alone: no atomics, the same call gives the same bits.
#pragma once
#include "pattern_plan.h"

namespace kpdi {

constexpr int RED_THREADS = 256;
constexpr int RED_COLS_SLICE = 128;     // rows of B that a lane walks: 512 slices x 1 - 4 workgroups for the mean pattern of a 256 x 256 map
constexpr int RED_RUNS_VECS = 16;       // 16-byte vectors of a slice per lane of the group
constexpr int RED_MAX_SLICES = 1024;    // per output: what the combine kernel adds
constexpr int RED_COMBINE_LANES = 16;   // lanes that share the partials of an output once there are more than ...
constexpr int RED_COMBINE_SERIAL = 32;  // ... this many: a lane alone adds that many in a row
constexpr int RED_COLS = 0, RED_RUNS = 1;
constexpr int RED_PHASE_SUM = 0, RED_PHASE_SUMSQ = 1, RED_PHASE_DEV2 = 2, RED_PHASE_MAX = 3, RED_PHASE_MIN = 4;

struct RedShape {
  int64_t A, R1, M, R2, B;
};

struct RedPlan {
  int regime;          // RED_COLS, RED_RUNS; -1: refused
  RedShape sh;
  int esize, vec;      // bytes of an element, elements of a 16-byte vector
  int64_t n_out, n_red;  // A * M * B outputs of R1 * R2 values each
  int64_t slice;       // consecutive r of one partial
  int n_slices;
  int combine_lanes;   // 1 or RED_COMBINE_LANES
  int64_t vb;          // RED_COLS: vectors of a row of B, the last one may be cut
  int64_t items;       // RED_COLS: A * M * vb lanes with work;  RED_RUNS: n_out * group
  int group;           // RED_RUNS: lanes that share an output
  unsigned grid_x, grid_y;  // workgroups of RED_THREADS: items, slices
  int passes;          // 2 for std / var of float patterns (the mean, then the squared deviations), else 1
  int planes;          // partials per (slice, output): 2 for std / var of integer patterns (sum x, sum x^2), else 1
  int out_dtype;       // KPDI_* of the result; uint64 / int64 sums are RED_OUT_U64 / RED_OUT_I64 below
  int out_esize;
  size_t partial_bytes, mean_off, out_off, workspace_bytes;  // partials | float64 means (passes == 2) | the result
};

constexpr int RED_OUT_U64 = 100, RED_OUT_I64 = 101;  // result dtypes that are no pattern dtype

PLAN_HD inline bool red_is_float(int dtype) { return dtype == KPDI_F32 || dtype == KPDI_F64; }
PLAN_HD inline bool red_is_signed(int dtype) { return dtype == KPDI_I8 || dtype == KPDI_I16; }

// NumPy's result dtype (2.2.6): sum -> uint64 / int64 / the float dtype; mean, std, var -> float64 / the float dtype;
// max, min -> the dtype
inline int red_out_dtype(int dtype, int op) {
  if (op == KPDI_REDUCE_MAX || op == KPDI_REDUCE_MIN || red_is_float(dtype)) return dtype;
  if (op == KPDI_REDUCE_SUM) return red_is_signed(dtype) ? RED_OUT_I64 : RED_OUT_U64;
  return KPDI_F64;
}

inline int red_out_bytes(int out_dtype) {
  return out_dtype == RED_OUT_U64 || out_dtype == RED_OUT_I64 ? 8 : pattern_dtype_bytes(out_dtype);
}

// dims (ny, nx, sy, sx) and the reduced axes (bit k: array axis k) as the five-group form above
inline RedShape red_shape(const int64_t dims[4], int axis_mask) {
  int64_t len[4];
  bool red[4];
  int n = 0;
  for (int k = 0; k < 4; ++k) {
    if (dims[k] == 1) continue;
    const bool r = (axis_mask >> k) & 1;
    if (n && red[n - 1] == r) len[n - 1] *= dims[k];
    else {
      len[n] = dims[k];
      red[n] = r;
      ++n;
    }
  }
  RedShape s{1, 1, 1, 1, 1};
  int g = 0;
  if (g < n && !red[g]) s.A = len[g++];
  const int left = n - g;  // R | R K | R K R | R K R K
  if (left <= 2) {
    if (left >= 1) s.R2 = len[g];
    if (left == 2) s.B = len[g + 1];
  } else {
    s.R1 = len[g];
    s.M = len[g + 1];
    s.R2 = len[g + 2];
    if (left == 4) s.B = len[g + 3];
  }
  return s;
}

// the smallest unit of r that a slice is made of
inline int64_t red_base_slice(int regime, int group, int vec) {
  return regime == RED_COLS ? RED_COLS_SLICE : (int64_t)group * vec * RED_RUNS_VECS;
}

inline RedPlan reduce_plan(int dtype, int op, int axis_mask, int64_t ny, int64_t nx, int64_t sy, int64_t sx) {
  RedPlan p{};
  p.regime = -1;
  p.esize = pattern_dtype_bytes(dtype);
  if (!p.esize || op < KPDI_REDUCE_SUM || op > KPDI_REDUCE_VAR || axis_mask < 1 || axis_mask > 15 || ny < 1 || nx < 1 ||
      sy < 1 || sx < 1)
    return p;
  const int64_t dims[4] = {ny, nx, sy, sx};
  p.sh = red_shape(dims, axis_mask);
  p.vec = 16 / p.esize;
  p.n_out = p.sh.A * p.sh.M * p.sh.B;
  p.n_red = p.sh.R1 * p.sh.R2;
  // sum x^2 of uint16 stays below 2^64 and float64(n) is exact far beyond this
  if (p.n_red >= ((int64_t)1 << 31)) return p;
  const int regime = p.sh.B > 1 ? RED_COLS : RED_RUNS;
  if (regime == RED_COLS) {
    p.vb = (p.sh.B + p.vec - 1) / p.vec;
    p.items = p.sh.A * p.sh.M * p.vb;
    p.group = 1;
  } else {
    const int64_t vectors = (p.sh.R2 + p.vec - 1) / p.vec;
    p.group = 1;
    while (p.group < 64 && p.group < vectors) p.group *= 2;
    p.items = p.n_out * p.group;
  }
  const int64_t base = red_base_slice(regime, p.group, p.vec);
  const int64_t units = (p.n_red + base - 1) / base;                       // slices of the smallest size
  p.slice = base * ((units + RED_MAX_SLICES - 1) / RED_MAX_SLICES);
  p.n_slices = (int)((p.n_red + p.slice - 1) / p.slice);
  p.combine_lanes = p.n_slices > RED_COMBINE_SERIAL ? RED_COMBINE_LANES : 1;
  const int64_t gx = (p.items + RED_THREADS - 1) / RED_THREADS;
  if (gx >= ((int64_t)1 << 31)) return p;
  p.grid_x = (unsigned)gx;
  p.grid_y = (unsigned)p.n_slices;
  const bool spread = op == KPDI_REDUCE_STD || op == KPDI_REDUCE_VAR;
  p.passes = spread && red_is_float(dtype) ? 2 : 1;
  p.planes = spread && !red_is_float(dtype) ? 2 : 1;
  p.out_dtype = red_out_dtype(dtype, op);
  p.out_esize = red_out_bytes(p.out_dtype);
  p.partial_bytes = (size_t)p.planes * p.n_slices * (size_t)p.n_out * 8;
  p.mean_off = p.partial_bytes;
  p.out_off = p.mean_off + (p.passes == 2 ? (size_t)p.n_out * 8 : 0);
  p.workspace_bytes = p.out_off + (size_t)p.n_out * p.out_esize;
  p.regime = regime;
  return p;
}

// ---- what the kernels and the host test both walk ---------------------------------------------------------------
// element (a, r1, m, r2, b) of the resident set
PLAN_HD inline int64_t red_element(const RedShape &s, int64_t a, int64_t r1, int64_t m, int64_t r2, int64_t b) {
  return (((a * s.R1 + r1) * s.M + m) * s.R2 + r2) * s.B + b;
}

// slice `s` is r in [lo, hi)
PLAN_HD inline void red_slice_bounds(int64_t n_red, int64_t slice, int s, int64_t *lo, int64_t *hi) {
  *lo = (int64_t)s * slice;
  *hi = *lo + slice < n_red ? *lo + slice : n_red;
}

// RED_COLS: lane `item` of the grid owns the `count` outputs (am, b0 ...) of row am = a * M + m
PLAN_HD inline void red_cols_item(int64_t item, int64_t vb, int vec, int64_t B, int64_t *am, int64_t *b0, int *count) {
  *am = item / vb;
  *b0 = (item - *am * vb) * vec;
  *count = B - *b0 < vec ? (int)(B - *b0) : vec;
}

// RED_RUNS: the lane of its group that owns vector `j` of a run's part
PLAN_HD inline int red_runs_lane(int64_t j, int group) { return (int)(j & (group - 1)); }

}  // namespace kpdi
