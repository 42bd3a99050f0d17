// geometrical.hip - geometrical simulations: the Kikuchi lines and zone axes of every map point on the detector
// (KikuchiPatternSimulator.on_detector, simulations/kikuchi_pattern_simulator.py:217-380; KikuchiPatternLine and
// KikuchiPatternZoneAxis, simulations/_kikuchi_pattern_features.py; _set_lines_detector_coordinates and
// _set_zone_axes_detector_coordinates, simulations/_kikuchi_pattern_simulation.py:468-534).  Float64, row vectors.
//
// A point's entry (geometrical_plan.h) holds K* and K with hkl_d = hkl K*, uvw_d = uvw K, the gnomonic bounds widened by
// one pixel, the offsets pcx / pcz * aspect_ratio and pcy / pcz, and the pixel scales.
//
// Visibility: per feature, bit 0 "z > 0 at some point", and for zone axes bit 1 "x / z and y / z inside the widened
// bounds of some point" (any sign of z; a comparison with NaN or inf is false, as NumPy's is).
//
// Coordinates, per (point, kept line) with (x, y, z) = hkl_d, R the largest gnomonic radius:
//   in_pattern = z > 0;  h = z / sqrt(x^2 + y^2)  (= tan(pi/2 - polar));  within = |h| < R and z > -1e-5
//   the reference's a1,2 = azimuth - pi +- acos(h / R) are never formed: with t = h / R, s = sqrt((1 - t)(1 + t)),
//   (cx, sy) = (x, y) / sqrt(x^2 + y^2):   cos a1 = -(cx t - sy s), sin a1 = -(sy t + cx s),
//                                          cos a2 = -(cx t + sy s), sin a2 = -(sy t - cx s)
//   gnomonic = R (cos a1, sin a1, cos a2, sin a2), NaN where not within; pixel x = (g + xoff) / x_scale,
//   pixel y = (-g + yoff) / y_scale.
// Per (point, kept zone axis): in_pattern = z > 0; (xg, yg) = (x, y) / z; within = sqrt(xg^2 + yg^2) < R and z > -1e-5;
//   gnomonic = (xg, yg), NaN where not within; pixel as above, NaN where the gnomonic point is NaN or outside the bounds.
//
// Vector stores only, no atomics, every output element written by exactly one lane.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "geometrical_plan.h"

#include <cmath>
#include <cstdlib>

namespace kpdi {

namespace {

struct GeoVisArgs {
  const double *vec;     // [m][3]
  const double *points;  // [n][GEO_ENTRY_DOUBLES]
  uint8_t *partial;      // [grid_y][m]
  int m, n, chunk, kind;
  int64_t n_chunks;
};

__global__ __launch_bounds__(GEO_THREADS) void geometrical_visibility_kernel(GeoVisArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[GEO_POINTS * GEO_VIS_DOUBLES];
  const int f = blockIdx.x * GEO_THREADS + threadIdx.x;
  const bool live = f < a.m;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (live) {
    const double *v = a.vec + (size_t)f * 3;
    v0 = v[0];
    v1 = v[1];
    v2 = v[2];
  }
  const int matrix = a.kind == GEO_ZONE_AXES ? 9 : 0;
  unsigned flags = 0;
  for (int64_t ci = blockIdx.y; ci < a.n_chunks; ci += gridDim.y) {
    const int64_t p0 = ci * a.chunk;
    const int len = a.n - p0 < a.chunk ? (int)(a.n - p0) : a.chunk;
    __syncthreads();  // the previous chunk has been read by every lane
    for (int i = threadIdx.x; i < len * GEO_VIS_DOUBLES; i += GEO_THREADS) {
      const int pt = i / GEO_VIS_DOUBLES, k = i % GEO_VIS_DOUBLES;
      const double *src = a.points + (size_t)(p0 + pt) * GEO_ENTRY_DOUBLES;
      tab[i] = k < 9 ? src[matrix + k] : k < 13 ? src[18 + (k - 9)] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < len; ++j) {
      const double *e = tab + j * GEO_VIS_DOUBLES;
      const double z = (v0 * e[2] + v1 * e[5]) + v2 * e[8];
      if (z > 0.0) flags |= GEO_FLAG_UPPER;
      if (a.kind == GEO_ZONE_AXES) {
        const double x = (v0 * e[0] + v1 * e[3]) + v2 * e[6];
        const double y = (v0 * e[1] + v1 * e[4]) + v2 * e[7];
        const double xg = x / z, yg = y / z;
        if (xg >= e[9] && xg <= e[10] && yg >= e[11] && yg <= e[12]) flags |= GEO_FLAG_INSIDE;
      }
    }
  }
  if (live) a.partial[(size_t)blockIdx.y * a.m + f] = (uint8_t)flags;
}

__global__ __launch_bounds__(GEO_THREADS) void geometrical_flags_or_kernel(const uint8_t *partial, uint8_t *flags, int m, int rows) {
  const int f = blockIdx.x * GEO_THREADS + threadIdx.x;
  if (f >= m) return;
  unsigned v = 0;
  for (int r = 0; r < rows; ++r) v |= partial[(size_t)r * m + f];
  flags[f] = (uint8_t)v;
}

struct GeoCoordArgs {
  const double *hkl;     // [m][3]
  const double *uvw;     // [z][3]
  const double *points;  // [points of this pass][GEO_ENTRY_DOUBLES]
  uint8_t *line_in;      // [points][m]
  double *line_gn;       // [points][m][4]
  double *line_px;       // [points][m][4]
  uint8_t *zone_in;      // [points][z]
  double *zone_gn;       // [points][z][2]
  double *zone_px;       // [points][z][2]
  int m, z, line_tiles, tiles;
  double r_gnomonic;
};

__global__ __launch_bounds__(GEO_THREADS) void geometrical_coordinates_kernel(GeoCoordArgs a) {
  const unsigned p = blockIdx.x / (unsigned)a.tiles;
  const int t = (int)(blockIdx.x % (unsigned)a.tiles);
  const double *e = a.points + (size_t)p * GEO_ENTRY_DOUBLES;  // the same address in every lane
  const double xoff = e[22], yoff = e[23], xs = e[24], ys = e[25];
  const double R = a.r_gnomonic;
  const double nan = __builtin_nan("");
  if (t < a.line_tiles) {
    const int f = t * GEO_THREADS + threadIdx.x;
    if (f >= a.m) return;
    const double *v = a.hkl + (size_t)f * 3;
    const double v0 = v[0], v1 = v[1], v2 = v[2];
    const double x = (v0 * e[0] + v1 * e[3]) + v2 * e[6];
    const double y = (v0 * e[1] + v1 * e[4]) + v2 * e[7];
    const double z = (v0 * e[2] + v1 * e[5]) + v2 * e[8];
    const double rho = sqrt(x * x + y * y);
    const double h = z / rho;
    const bool within = fabs(h) < R && z > GEO_FULL_UPPER;
    double4 gn = make_double4(nan, nan, nan, nan), px = gn;
    if (within) {
      const double tt = h / R;
      const double s = sqrt((1.0 - tt) * (1.0 + tt));
      const double cx = x / rho, sy = y / rho;
      gn.x = R * -(cx * tt - sy * s);
      gn.y = R * -(sy * tt + cx * s);
      gn.z = R * -(cx * tt + sy * s);
      gn.w = R * -(sy * tt - cx * s);
      px.x = (gn.x + xoff) / xs;
      px.y = (-gn.y + yoff) / ys;
      px.z = (gn.z + xoff) / xs;
      px.w = (-gn.w + yoff) / ys;
    }
    const size_t o = (size_t)p * a.m + f;
    a.line_in[o] = z > 0.0 ? 1 : 0;
    reinterpret_cast<double4 *>(a.line_gn)[o] = gn;
    reinterpret_cast<double4 *>(a.line_px)[o] = px;
  } else {
    const int f = (t - a.line_tiles) * GEO_THREADS + threadIdx.x;
    if (f >= a.z) return;
    const double *v = a.uvw + (size_t)f * 3;
    const double v0 = v[0], v1 = v[1], v2 = v[2];
    const double x = (v0 * e[9] + v1 * e[12]) + v2 * e[15];
    const double y = (v0 * e[10] + v1 * e[13]) + v2 * e[16];
    const double z = (v0 * e[11] + v1 * e[14]) + v2 * e[17];
    const double xg = x / z, yg = y / z;
    const bool within = sqrt(xg * xg + yg * yg) < R && z > GEO_FULL_UPPER;
    const bool inside = within && xg >= e[18] && xg <= e[19] && yg >= e[20] && yg <= e[21];
    double2 gn = make_double2(nan, nan), px = gn;
    if (within) gn = make_double2(xg, yg);
    if (inside) px = make_double2((xg + xoff) / xs, (-yg + yoff) / ys);
    const size_t o = (size_t)p * a.z + f;
    a.zone_in[o] = z > 0.0 ? 1 : 0;
    reinterpret_cast<double2 *>(a.zone_gn)[o] = gn;
    reinterpret_cast<double2 *>(a.zone_px)[o] = px;
  }
}

int forced_chunk() {
  if (const char *e = getenv("KPDI_GEOMETRICAL_CHUNK")) return atoi(e);  // tests: chunk edges at small point counts
  return 0;
}

}  // namespace

GeoVisPlan geometrical_visibility_plan(int64_t m, int64_t n_points) { return geo_visibility_plan(m, n_points, forced_chunk()); }

GeoCoordPlan geometrical_coord_plan(int64_t m, int64_t z, int64_t n_points, size_t budget_bytes) {
  return geo_coord_plan(m, z, n_points, budget_bytes, forced_chunk());
}

hipError_t launch_geometrical_visibility(const GeoVisLaunch &l, hipStream_t s) {
  const GeoVisPlan plan = geometrical_visibility_plan(l.m, l.n_points);
  if (!plan.ok || !l.vec || !l.points || !l.partial || !l.flags || (l.kind != GEO_LINES && l.kind != GEO_ZONE_AXES))
    return hipErrorInvalidValue;
  GeoVisArgs a{};
  a.vec = l.vec;
  a.points = l.points;
  a.partial = l.partial;
  a.m = (int)l.m;
  a.n = (int)l.n_points;
  a.chunk = plan.chunk;
  a.kind = l.kind;
  a.n_chunks = plan.n_chunks;
  hipLaunchKernelGGL(geometrical_visibility_kernel, dim3((unsigned)plan.tiles, (unsigned)plan.grid_y), dim3(GEO_THREADS), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(geometrical_flags_or_kernel, dim3((unsigned)plan.tiles), dim3(GEO_THREADS), 0, s, l.partial, l.flags, (int)l.m,
                     plan.grid_y);
  return hipGetLastError();
}

hipError_t launch_geometrical_coordinates(const GeoCoordLaunch &l, hipStream_t s) {
  if (l.m < 1 || l.z < 0 || l.points_in_pass < 1 || !l.hkl || !l.points || !l.line_in || !l.line_gn || !l.line_px ||
      (l.z > 0 && (!l.uvw || !l.zone_in || !l.zone_gn || !l.zone_px)))
    return hipErrorInvalidValue;
  const int line_tiles = (int)((l.m + GEO_THREADS - 1) / GEO_THREADS), zone_tiles = (int)((l.z + GEO_THREADS - 1) / GEO_THREADS);
  const int64_t blocks = l.points_in_pass * (line_tiles + zone_tiles);
  if (blocks > INT32_MAX) return hipErrorInvalidValue;
  GeoCoordArgs a{};
  a.hkl = l.hkl;
  a.uvw = l.uvw;
  a.points = l.points;
  a.line_in = l.line_in;
  a.line_gn = l.line_gn;
  a.line_px = l.line_px;
  a.zone_in = l.zone_in;
  a.zone_gn = l.zone_gn;
  a.zone_px = l.zone_px;
  a.m = (int)l.m;
  a.z = (int)l.z;
  a.line_tiles = line_tiles;
  a.tiles = line_tiles + zone_tiles;
  a.r_gnomonic = l.r_gnomonic;
  hipLaunchKernelGGL(geometrical_coordinates_kernel, dim3((unsigned)blocks), dim3(GEO_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace kpdi
