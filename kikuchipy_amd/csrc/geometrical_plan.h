// geometrical_plan.h - how geometrical.hip lays a geometrical simulation (KikuchiPatternSimulator.on_detector,
// simulations/kikuchi_pattern_simulator.py:217-380) on the chip, and the per-point table both kernels read: pure
// functions, no HIP call (tests/test_host_geometrical.py compiles this header with the host compiler).
//
// A feature is a Kikuchi line (a reflector hkl) or a zone axis (a direction uvw); a point is one map point: one rotation
// and one projection centre.  Everything about a point that does not depend on the feature is formed ONCE per point, on
// the host, into an entry of GEO_ENTRY_DOUBLES float64 (geo_point_entry): the two 3 x 3 matrices that take row vectors
// hkl / uvw to detector coordinates and the point's gnomonic bounds, offsets and scales.
//
// Visibility pass: GEO_THREADS features per workgroup (blockIdx.x, one feature per lane) x point chunks (blockIdx.y and
// on in steps of gridDim.y); a chunk's matrices and bounds are staged in LDS (GEO_VIS_DOUBLES per point) and read by every
// lane at the same address, a broadcast.  Row blockIdx.y of the partial flags gets the OR over that row's chunks; a second
// kernel ORs the rows.  OR is order-free: the flags do not depend on the chunk length or the launch.
//
// Coordinate pass: one workgroup per (point, tile of GEO_THREADS kept features), the line tiles of a point first, then
// its zone-axis tiles; consecutive lanes take consecutive features, outputs are (point, feature, 4 or 2), so a wave's
// stores cover one contiguous span.  The map is walked in passes of `points` points, sized from free device memory, so
// the outputs of a large map are never resident all at once.
#pragma once
#include <cstddef>
#include <cstdint>

namespace kpdi {

constexpr int GEO_THREADS = 256;        // features per workgroup
constexpr int GEO_POINTS = 64;          // points staged in LDS at once by the visibility pass
constexpr int GEO_ENTRY_DOUBLES = 32;   // per point: K*[9] K[9] x0 x1 y0 y1 (widened) xoff yoff x_scale y_scale, 6 pad
constexpr int GEO_VIS_DOUBLES = 16;     // of those in LDS: one matrix [9], the widened bounds [4], 3 pad
constexpr size_t GEO_LDS_BYTES = (size_t)GEO_POINTS * GEO_VIS_DOUBLES * sizeof(double);  // 8 KiB
constexpr int GEO_MAX_GRID_Y = 256;     // rows of partial flags
constexpr int GEO_PC_DOUBLES = 8;       // a projection centre as the caller gives it: x0 x1 y0 y1 (widened) xoff yoff x_scale y_scale
constexpr int GEO_LINES = 0, GEO_ZONE_AXES = 1;
constexpr int GEO_FLAG_UPPER = 1, GEO_FLAG_INSIDE = 2;
constexpr double GEO_FULL_UPPER = -1e-5;  // z > this: `is_full_upper` of simulations/_kikuchi_pattern_features.py:49
constexpr size_t GEO_LINE_BYTES = 1 + 2 * 4 * sizeof(double);  // per (point, line): in_pattern, gnomonic[4], pixel[4]
constexpr size_t GEO_ZONE_BYTES = 1 + 2 * 2 * sizeof(double);  // per (point, zone axis): in_pattern, gnomonic[2], pixel[2]
constexpr size_t GEO_PASS_BYTES = (size_t)256 << 20;           // most output bytes of one pass (also the staging copy's)

struct GeoVisPlan {
  int ok;
  int tiles;          // feature tiles (grid x)
  int last_features;  // lanes of the last tile that own a feature (GEO_THREADS when it is full)
  int chunk;          // points per LDS stage
  int64_t n_chunks;
  int tail;           // points of the last stage (chunk when it is full)
  int grid_y;         // rows of partial flags: min(n_chunks, GEO_MAX_GRID_Y)
  size_t lds_bytes;   // static: the full GEO_POINTS whatever `chunk`
};

// `force_chunk`: 0, or a shorter chunk (tests: chunk edges at small point counts); clamped to [1, GEO_POINTS]
inline GeoVisPlan geo_visibility_plan(int64_t m, int64_t n_points, int force_chunk = 0) {
  GeoVisPlan p{};
  if (m < 1 || m > INT32_MAX || n_points < 1 || n_points > INT32_MAX) return p;
  p.tiles = (int)((m + GEO_THREADS - 1) / GEO_THREADS);
  p.last_features = m % GEO_THREADS ? (int)(m % GEO_THREADS) : GEO_THREADS;
  p.chunk = force_chunk < 1 ? GEO_POINTS : force_chunk > GEO_POINTS ? GEO_POINTS : force_chunk;
  p.n_chunks = (n_points + p.chunk - 1) / p.chunk;
  p.tail = n_points % p.chunk ? (int)(n_points % p.chunk) : p.chunk;
  p.grid_y = p.n_chunks < GEO_MAX_GRID_Y ? (int)p.n_chunks : GEO_MAX_GRID_Y;
  p.lds_bytes = GEO_LDS_BYTES;
  p.ok = 1;
  return p;
}

struct GeoCoordPlan {
  int ok;
  int line_tiles, zone_tiles;  // per point; a workgroup is (point, tile), the line tiles first
  int tiles;                   // their sum
  size_t bytes_per_point;      // of all six outputs
  int64_t points;              // per pass
  int64_t n_passes;
  int64_t tail;                // points of the last pass (points when it is full)
};

// `budget_bytes`: what the outputs of one pass may take (from free device memory); `force_points`: 0, or the points of
// a pass (tests).  m lines (at least one), z zone axes (may be none).  A pass launches points * tiles workgroups in a 1-D
// grid, kept below 2^31.
inline GeoCoordPlan geo_coord_plan(int64_t m, int64_t z, int64_t n_points, size_t budget_bytes, int force_points = 0) {
  GeoCoordPlan p{};
  if (m < 1 || m > INT32_MAX || z < 0 || z > INT32_MAX || n_points < 1 || n_points > INT32_MAX) return p;
  p.line_tiles = (int)((m + GEO_THREADS - 1) / GEO_THREADS);
  p.zone_tiles = (int)((z + GEO_THREADS - 1) / GEO_THREADS);
  p.tiles = p.line_tiles + p.zone_tiles;
  p.bytes_per_point = (size_t)m * GEO_LINE_BYTES + (size_t)z * GEO_ZONE_BYTES;
  const size_t budget = budget_bytes < GEO_PASS_BYTES ? budget_bytes : GEO_PASS_BYTES;
  int64_t points = (int64_t)(budget / p.bytes_per_point);
  if (force_points >= 1) points = force_points;
  const int64_t grid_cap = (int64_t)INT32_MAX / p.tiles;
  if (points > grid_cap) points = grid_cap;
  if (points > n_points) points = n_points;
  if (points < 1) points = 1;
  p.points = points;
  p.n_passes = (n_points + points - 1) / points;
  p.tail = n_points % points ? n_points % points : points;
  p.ok = 1;
  return p;
}

// rotation matrix of a unit quaternion (a, b, c, d), row-major, the matrix of `rotate_vector` (_utils/numba.py:62-81; the
// coefficients of csrc/projection.h, rot_coeff) and of orix's Rotation.to_matrix(): v' = U v
inline void geo_rotation_matrix(const double *q, double *u) {
  const double a = q[0], b = q[1], c = q[2], d = q[3];
  const double aa = a * a, bb = b * b, cc = c * c, dd = d * d;
  u[0] = aa + bb - cc - dd;  u[1] = 2.0 * (b * c - a * d);  u[2] = 2.0 * (a * c + b * d);
  u[3] = 2.0 * (a * d + b * c);  u[4] = aa - bb + cc - dd;  u[5] = 2.0 * (c * d - a * b);
  u[6] = 2.0 * (b * d - a * c);  u[7] = 2.0 * (a * b + c * d);  u[8] = aa - bb - cc + dd;
}

inline void geo_matmul3(const double *a, const double *b, double *c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// the entry of one point: U_os = U_o U_s, K* = A* U_os (hkl_d = hkl K*), K = A U_os (uvw_d = uvw K), row vectors
// (simulations/kikuchi_pattern_simulator.py:259-306); `a_star` / `a_direct` may be NULL (that matrix is zeroed)
inline void geo_point_entry(const double *q, const double *u_s, const double *a_star, const double *a_direct, const double *pc,
                            double *e) {
  double u_o[9], u_os[9];
  geo_rotation_matrix(q, u_o);
  geo_matmul3(u_o, u_s, u_os);
  for (int i = 0; i < GEO_ENTRY_DOUBLES; ++i) e[i] = 0.0;
  if (a_star) geo_matmul3(a_star, u_os, e);
  if (a_direct) geo_matmul3(a_direct, u_os, e + 9);
  for (int i = 0; i < GEO_PC_DOUBLES; ++i) e[18 + i] = pc[i];
}

}  // namespace kpdi
