// kinematical_plan.h - how kinematical.hip lays a kinematical master pattern on the chip: pure functions of the half
// size, the reflector count and the hemispheres, no HIP call (tests/test_host_kinematical.py compiles this header with
// the host compiler and checks the geometry, the chunking, the LDS budget and the acos screen).
//
// One thread per pixel of the (2 half_size + 1)^2 stereographic grid, KIN_THREADS of them per workgroup; blockIdx.y is
// the hemisphere, so "both" is one launch.  The reflector table is the same for every lane: a workgroup stages it in LDS
// `chunk` reflectors at a time (KIN_CHUNK unless a developer switch shortens it) and every lane walks a chunk in rising
// reflector index, all lanes reading the same address (a broadcast, no bank conflict).  A pixel's sum therefore has ONE
// order, rising reflector index, whatever the chunk length or the launch looks like.
//
// The acos screen: the band test of a pair with D > 1e-7 is theta1 <= acos(D), theta1 = pi/2 - theta (acos(D) <= pi/2
// holds for every such D).  With c = cos(theta1) rounded to float64, a pair with D >= c + KIN_SCREEN is outside and one
// with D <= c - KIN_SCREEN inside whatever the last bits of acos are; only pairs between the two thresholds evaluate
// acos and compare as the reference does (the argument: DESIGN.md section 17).  The screen holds for theta1 in [0, pi];
// any other theta (NaN included) gets thresholds of -inf / +inf, so all its pairs with D > 1e-7 take the acos path.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace kpdi {

constexpr int KIN_THREADS = 256;          // pixels per workgroup
constexpr int KIN_CHUNK = 256;            // reflectors staged in LDS at once
constexpr int KIN_ENTRY_DOUBLES = 8;      // ux uy uz I | lo hi theta1 (pad): two 32-byte halves, the second read on demand
constexpr size_t KIN_LDS_BYTES = (size_t)KIN_CHUNK * KIN_ENTRY_DOUBLES * sizeof(double);  // 16 KiB: 8 workgroups per CU fit
constexpr int KIN_MAX_HALF_SIZE = 4096;   // 8193^2 pixels: 1.6 GB of directions, 1 GB of output for both hemispheres
constexpr double KIN_HALF_WIDTH = 1e-7;   // |D| <= this: the pixel lies on the band's centre line, half the intensity
constexpr double KIN_SCREEN = 1e-6;       // margin of the acos screen in D
constexpr int KIN_UPPER = 0, KIN_LOWER = 1, KIN_BOTH = 2;

struct KinPlan {
  int ok;
  int size;            // pixels per side
  int64_t pixels;      // per hemisphere
  int hemispheres;     // 1 or 2
  int grid_x, grid_y;  // workgroups: pixels, hemispheres
  int threads;
  int last_threads;    // lanes of the last workgroup that own a pixel (KIN_THREADS when it is full)
  int chunk;           // reflectors per LDS stage
  int n_chunks;
  int tail;            // reflectors of the last stage (chunk when it is full)
  size_t lds_bytes;    // of one workgroup (static: the full KIN_CHUNK whatever `chunk`)
};

inline int kin_hemispheres(int code) { return code == KIN_BOTH ? 2 : (code == KIN_UPPER || code == KIN_LOWER) ? 1 : 0; }
// z of the direction of hemisphere `h` of a launch is zsign * (the upper hemisphere's z): -pole of the reference
inline double kin_zsign(int code, int h) { return (code == KIN_LOWER || (code == KIN_BOTH && h == 1)) ? -1.0 : 1.0; }

// `force_chunk`: 0, or a shorter chunk (tests: chunk boundaries at small reflector counts); clamped to [1, KIN_CHUNK]
inline KinPlan kin_plan(int64_t m, int half_size, int hemispheres, int force_chunk = 0) {
  KinPlan p{};
  const int nh = kin_hemispheres(hemispheres);
  if (m < 1 || m > INT32_MAX || half_size < 0 || half_size > KIN_MAX_HALF_SIZE || nh == 0) return p;
  p.size = 2 * half_size + 1;
  p.pixels = (int64_t)p.size * p.size;
  p.hemispheres = nh;
  p.threads = KIN_THREADS;
  p.grid_x = (int)((p.pixels + KIN_THREADS - 1) / KIN_THREADS);
  p.grid_y = nh;
  p.last_threads = p.pixels % KIN_THREADS ? (int)(p.pixels % KIN_THREADS) : KIN_THREADS;
  p.chunk = force_chunk < 1 ? KIN_CHUNK : force_chunk > KIN_CHUNK ? KIN_CHUNK : force_chunk;
  p.n_chunks = (int)((m + p.chunk - 1) / p.chunk);
  p.tail = m % p.chunk ? (int)(m % p.chunk) : p.chunk;
  p.lds_bytes = KIN_LDS_BYTES;
  p.ok = 1;
  return p;
}

// the acos screen of one reflector from theta1 = pi/2 - theta: D <= *lo is inside the band, D >= *hi outside
inline void kin_screen(double theta1, double *lo, double *hi) {
  if (theta1 >= 0.0 && theta1 <= 3.141592653589793) {
    const double c = std::cos(theta1);
    *lo = c - KIN_SCREEN;
    *hi = c + KIN_SCREEN;
  } else {
    *lo = -std::numeric_limits<double>::infinity();
    *hi = std::numeric_limits<double>::infinity();
  }
}

// direction of the grid's pixel (row, col) on the upper hemisphere, with NumPy's operations one by one:
// arr = np.linspace(-1, 1, size) is arange(size) * (2.0 / (size - 1)) + (-1.0) with arr[-1] = 1.0 (size 1: [-1.0]);
// the inverse stereographic projection is (2 x / d, 2 y / d, (1 - x^2 - y^2) / d), d = 1 + x^2 + y^2, x = arr[col],
// y = arr[row].  Compiled without contraction (-ffp-contract=off) every operation rounds as NumPy's does.
inline double kin_axis(int i, int size) {
  if (size == 1) return -1.0;
  if (i == size - 1) return 1.0;
  const double step = 2.0 / (double)(size - 1);
  return (double)i * step + -1.0;
}
inline void kin_direction(double x, double y, double *v) {
  const double xx = x * x, yy = y * y;
  const double d = (1.0 + xx) + yy;
  v[0] = (2.0 * x) / d;
  v[1] = (2.0 * y) / d;
  v[2] = ((1.0 - xx) - yy) / d;
}

}  // namespace kpdi
