// orientations_plan.h - what orientations.hip computes for one pair of orientations, one orientation or one map point, and
// how it lays the work on the chip: pure functions, no HIP call, `__host__ __device__` under hipcc and plain inline
// functions under a host compiler (tests/test_host_orientations.py compiles this header with the host compiler).
// Definitions: DESIGN.md section 25.
//
// Quaternions are (a, b, c, d); an orientation g maps lab to crystal; its equivalents under the operations S of a rotation
// group are s g.  A row is normalised first, q / sqrt(a a + b b + c c + d d); a row whose norm is not a positive finite
// number (a non-finite component, zeros, squares that leave float64's range) becomes four NaNs and every result it
// enters is NaN.
//
// The disorientation angle of g1 under S1 and g2 under S2: the candidates are (s1 g1, s2 g2), index s1 n2 + s2; the one
// with the largest |(s1 g1) . (s2 g2)| wins, the lowest index among equal maxima; the winner is evaluated again as the
// product (s2 g2) (s1 g1)^-1 = (w, v) and the angle is 2 atan2(|v|, |w|) - never 2 acos of the maximum, which loses
// half of the digits at small angles.  Equal groups pass S1 = {1}: one side's equivalents suffice.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define ORI_HD __host__ __device__ inline
#else
#define ORI_HD inline
#endif

namespace kpdi {

constexpr int ORI_MAX_OPS = 24;        // the order of 432: no rotation group has more operations
constexpr int ORI_THREADS = 256;       // per workgroup of every kernel here (4 waves)
constexpr int ORI_TILE_I = 32;         // rows (first set) of an output tile of the outer kernel
constexpr int ORI_TILE_J = 32;         // columns (second set): 2 x 2 blocks of the 16 x 16 x 4 float64 MFMA, one per wave
constexpr int ORI_MFMA = 16;           // side of an MFMA block
constexpr int ORI_MAX_DIMS = 8;        // leading axes of a broadcast pair call
constexpr int ORI_MAX_OFFSETS = 1024;  // neighbours under a KAM window
constexpr int64_t ORI_MAX_TILES = 2147483647LL;  // workgroups of one launch (a grid's x dimension)
constexpr double ORI_DEGREES = 57.29577951308232;  // 180 / pi

// the operations of a rotation group, passed to the kernels by value (24 x 32 B = 768 B of kernel arguments)
struct OriOps {
  int n;
  double q[ORI_MAX_OPS][4];
};

// the leading axes of a broadcast pair call: strides in quaternions, 0 where an input is broadcast
struct OriShape {
  int nd;
  int64_t dim[ORI_MAX_DIMS], stride1[ORI_MAX_DIMS], stride2[ORI_MAX_DIMS];
};

// Hamilton product p q
ORI_HD void ori_product(const double *p, const double *q, double *r) {
  r[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3];
  r[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
  r[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1];
  r[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}

// the unit quaternion of a row, or four NaNs
ORI_HD void ori_normalise(const double *q, double *g) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const bool ok = n > 0.0 && n <= 1.7976931348623157e308;
  const double bad = nan("");
  for (int k = 0; k < 4; ++k) g[k] = ok ? q[k] / n : bad;
}

ORI_HD double ori_dot(const double *p, const double *q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2] + p[3] * q[3]; }

// the rotation angle of e2 e1^-1 for unit e1, e2: 2 atan2(|v|, |w|)
ORI_HD double ori_angle(const double *e1, const double *e2) {
  const double conj1[4] = {e1[0], -e1[1], -e1[2], -e1[3]};
  double r[4];
  ori_product(e2, conj1, r);
  return 2.0 * atan2(sqrt(r[1] * r[1] + r[2] * r[2] + r[3] * r[3]), fabs(r[0]));
}

// the disorientation angle of two NORMALISED rows (radians); *winner = s1 n2 + s2 of the candidate taken
ORI_HD double ori_pair_angle(const double *g1, const double *g2, const OriOps &ops1, const OriOps &ops2, int *winner) {
  double best = -1.0, b1[4] = {g1[0], g1[1], g1[2], g1[3]}, b2[4] = {g2[0], g2[1], g2[2], g2[3]};
  int at = 0;
  for (int s1 = 0; s1 < ops1.n; ++s1) {
    double e1[4];
    ori_product(ops1.q[s1], g1, e1);
    for (int s2 = 0; s2 < ops2.n; ++s2) {
      double e2[4];
      ori_product(ops2.q[s2], g2, e2);
      const double d = fabs(ori_dot(e1, e2));
      if (d > best || (s1 == 0 && s2 == 0)) {  // (the first candidate is taken whatever it is: NaN rows)
        best = d;
        at = s1 * ops2.n + s2;
        for (int k = 0; k < 4; ++k) {
          b1[k] = e1[k];
          b2[k] = e2[k];
        }
      }
    }
  }
  if (winner) *winner = at;
  return ori_angle(b1, b2);
}

// zone reduction of one raw row: the equivalent s g with the largest |w|, the lowest index among equal maxima, with
// w >= 0 (a half turn: its first non-zero component positive).  Returns the operation's index, -1 for a NaN row.
ORI_HD int ori_reduce(const double *q, const OriOps &ops, double *out) {
  double g[4];
  ori_normalise(q, g);
  if (!(g[0] == g[0])) {
    for (int k = 0; k < 4; ++k) out[k] = g[k];
    return -1;
  }
  double best = -1.0;
  int at = 0;
  for (int s = 0; s < ops.n; ++s) {
    double e[4];
    ori_product(ops.q[s], g, e);
    if (fabs(e[0]) > best) {
      best = fabs(e[0]);
      at = s;
      for (int k = 0; k < 4; ++k) out[k] = e[k];
    }
  }
  double lead = 0.0;
  for (int k = 3; k >= 0; --k) lead = out[k] != 0.0 ? out[k] : lead;  // the first non-zero component
  if (lead < 0.0)
    for (int k = 0; k < 4; ++k) out[k] = -out[k];
  return at;
}

// output element of a broadcast pair call -> the rows of the two inputs
ORI_HD void ori_pair_rows(int64_t p, const OriShape &s, int64_t *row1, int64_t *row2) {
  int64_t r1 = 0, r2 = 0;
  for (int d = s.nd - 1; d >= 0; --d) {
    const int64_t i = p % s.dim[d];
    p /= s.dim[d];
    r1 += i * s.stride1[d];
    r2 += i * s.stride2[d];
  }
  *row1 = r1;
  *row2 = r2;
}

// KAM of one map point: the mean disorientation angle (radians) to the neighbours at `offsets` (n x (dy, dx), in window
// order), float64 sum in that order.  Left out: neighbours outside the map, outside `in_data` (nullptr: all inside), or
// further than `max_angle` (negative: no limit).  NaN for a point outside the data or without a neighbour left.
ORI_HD double ori_kam_point(const double *rot, int ny, int nx, int y, int x, const OriOps &one, const OriOps &ops,
                            const int32_t *offsets, int n_offsets, const uint8_t *in_data, double max_angle) {
  const int64_t p = (int64_t)y * nx + x;
  if (in_data && !in_data[p]) return nan("");
  double g[4];
  ori_normalise(rot + 4 * p, g);
  double sum = 0.0;
  int count = 0;
  for (int j = 0; j < n_offsets; ++j) {
    const int yy = y + offsets[2 * j], xx = x + offsets[2 * j + 1];
    if (yy < 0 || yy >= ny || xx < 0 || xx >= nx) continue;
    const int64_t pn = (int64_t)yy * nx + xx;
    if (in_data && !in_data[pn]) continue;
    double h[4];
    ori_normalise(rot + 4 * pn, h);
    const double w = ori_pair_angle(g, h, one, ops, nullptr);
    if (max_angle >= 0.0 && w > max_angle) continue;
    sum += w;
    ++count;
  }
  return count > 0 ? sum / (double)count : nan("");
}

// ---- launch arithmetic ----------------------------------------------------------------------------------------------------
ORI_HD int64_t ori_blocks(int64_t items) { return (items + ORI_THREADS - 1) / ORI_THREADS; }

// The outer kernel: a workgroup owns ORI_TILE_I x ORI_TILE_J outputs; tile t of a pass covers the rows
// (t / tiles_j) ORI_TILE_I ... of the pass and the columns (t % tiles_j) ORI_TILE_J ...  The output of all n rows may not
// fit in device memory: it is walked in passes of `pass_rows` rows (a multiple of the tile's rows unless forced), each
// pass one launch and one copy to the host.
struct OriOuterPlan {
  int ok;
  int64_t n, m;
  int64_t pass_rows;   // rows of a full pass
  int64_t n_passes;
  int64_t tail_rows;   // rows of the last pass
  int64_t tiles_j;     // tiles along the columns
  int64_t pass_tiles;  // workgroups of a full pass
  size_t pass_bytes;   // output of a full pass
};

// `budget_bytes`: device memory the output of one pass may take; `forced_rows` > 0: that many rows per pass
ORI_HD OriOuterPlan ori_outer_plan(int64_t n, int64_t m, int elem_bytes, size_t budget_bytes, int64_t forced_rows) {
  OriOuterPlan p{};
  if (n < 1 || m < 1 || (elem_bytes != 4 && elem_bytes != 8)) return p;
  p.n = n;
  p.m = m;
  p.tiles_j = (m + ORI_TILE_J - 1) / ORI_TILE_J;
  const size_t row_bytes = (size_t)m * (size_t)elem_bytes;
  int64_t rows = (int64_t)(budget_bytes / row_bytes);
  if (rows > n) rows = n;
  const int64_t by_grid = ORI_MAX_TILES / p.tiles_j * ORI_TILE_I;  // a pass is one launch
  if (rows > by_grid) rows = by_grid;
  if (rows >= ORI_TILE_I && rows < n) rows -= rows % ORI_TILE_I;
  if (forced_rows > 0) rows = forced_rows < n ? forced_rows : n;
  if (rows < 1 || rows > by_grid) return p;  // not even one row fits
  p.pass_rows = rows;
  p.n_passes = (n + rows - 1) / rows;
  p.tail_rows = n - (p.n_passes - 1) * rows;
  p.pass_tiles = (rows + ORI_TILE_I - 1) / ORI_TILE_I * p.tiles_j;
  p.pass_bytes = (size_t)rows * row_bytes;
  p.ok = 1;
  return p;
}

// tile of a pass -> its first row (within the pass) and first column
ORI_HD void ori_tile_origin(int64_t tile, int64_t tiles_j, int64_t *row0, int64_t *col0) {
  *row0 = tile / tiles_j * ORI_TILE_I;
  *col0 = tile % tiles_j * ORI_TILE_J;
}

// element (row of the pass, column) of a pass's output: 64-bit, a pass may hold more than 2^32 outputs
ORI_HD int64_t ori_out_index(int64_t row, int64_t col, int64_t m) { return row * m + col; }

}  // namespace kpdi
