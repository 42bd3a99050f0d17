// sampling_plan.h - what sampling.hip computes for one point of the cubochoric grid, and how it lays the grid on the chip:
// pure functions, no HIP call, `__host__ __device__` under hipcc and plain inline functions under a host compiler
// (tests/test_host_sampling.py compiles this header with the host compiler and checks the grid decode, the launch
// arithmetic and the kept flags against the NumPy sampler of kikuchipy_amd/sampling.py).
//
// The grid: (2 n + 1)^3 points of the cube of semi-edge pi^(2/3) / 2, point p = (ix (2n+1) + iy) (2n+1) + iz, x slowest,
// coordinate (i - n) * (semi_edge / n) as NumPy's arange(-n, n + 1) * (semi_edge / n) gives it.  p is 64-bit:
// (2 n + 1)^3 passes 2^31 at n = 645.
//
// A point -> homochoric ball (Rosca, Morawiec & De Graef 2014, the operations of cubochoric_to_homochoric one by one) ->
// |ho| = (3/4 (w - sin w))^(1/3) inverted for w in [0, pi] by 60 bisection steps on w - sin w against 4/3 |ho|^3 (the
// host's bisection without its cube root per step) -> q = (cos(w/2), ho / |ho| sin(w/2)), q0 >= 0.
//
// The face rule: q is kept iff |q_v . a| <= tan(omega/4) q0 + SMP_FACE_SLACK for every face (a, tan(omega/4)) of the
// rotation group (fundamental_zone_faces of kikuchipy_amd/sampling.py).  Every decision of the grids in use is either a
// point ON a face (the slack keeps it) or at least 1e-6 from its threshold, so the last bits of sin / cos do not decide.
//
// The launch: SMP_THREADS consecutive points per workgroup, one per thread; the kept points of a workgroup are counted,
// the counts are scanned (exclusive, 64-bit) and each workgroup writes its kept quaternions from its offset on, in
// point order: the output has the host's lexicographic order without any atomic.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SMP_HD __host__ __device__ inline
#else
#define SMP_HD inline
#endif

namespace kpdi {

constexpr int SMP_THREADS = 256;        // points per workgroup (4 waves)
constexpr int SMP_WAVES = SMP_THREADS / 64;
constexpr int SMP_SCAN_THREADS = 1024;  // of the one workgroup that scans the counts
constexpr int SMP_MAX_FACES = 23;       // the non-identity operations of 432: no rotation group has more faces
constexpr int SMP_FACE_DOUBLES = 4;     // ax ay az tan(omega/4)
constexpr int SMP_MAX_STEPS = 2048;     // 4097^3 = 6.9e10 points, 2.7e8 workgroups (0.06 degrees; 1 degree is n = 137)
constexpr int SMP_BISECTIONS = 60;      // the host's: the bracket ends pi 2^-60 wide
constexpr double SMP_FACE_SLACK = 1e-9;
constexpr double SMP_SEMI_EDGE = 1.0725146985555127;  // np.pi ** (2 / 3) / 2

// the face table, passed to the kernels by value (23 x 32 B = 736 B of kernel arguments, read through the scalar cache)
struct SmpFaces {
  int n;
  double f[SMP_MAX_FACES][SMP_FACE_DOUBLES];
};

struct SmpPlan {
  int ok;
  int steps;           // n
  int side;            // 2 n + 1
  int64_t points;      // side^3
  int64_t blocks;      // workgroups of the count and emit passes (fits a grid's x dimension)
  int threads;
  int last_threads;    // lanes of the last workgroup that own a point (SMP_THREADS when it is full)
  int scan_threads;
  int64_t scan_rounds; // SMP_SCAN_THREADS counts per round of the scan's one workgroup
  size_t count_bytes;  // one uint32 per workgroup
  size_t offset_bytes; // one int64 per workgroup, and the total after them
};

SMP_HD SmpPlan smp_plan(int steps) {
  SmpPlan p{};
  if (steps < 1 || steps > SMP_MAX_STEPS) return p;
  p.steps = steps;
  p.side = 2 * steps + 1;
  p.points = (int64_t)p.side * p.side * p.side;
  p.threads = SMP_THREADS;
  p.blocks = (p.points + SMP_THREADS - 1) / SMP_THREADS;
  p.last_threads = p.points % SMP_THREADS ? (int)(p.points % SMP_THREADS) : SMP_THREADS;
  p.scan_threads = SMP_SCAN_THREADS;
  p.scan_rounds = (p.blocks + SMP_SCAN_THREADS - 1) / SMP_SCAN_THREADS;
  p.count_bytes = (size_t)p.blocks * sizeof(uint32_t);
  p.offset_bytes = ((size_t)p.blocks + 1) * sizeof(int64_t);
  p.ok = 1;
  return p;
}

// point index -> (ix, iy, iz), x slowest
SMP_HD void smp_decode(int64_t p, int side, int *ix, int *iy, int *iz) {
  const int64_t plane = (int64_t)side * side;
  *ix = (int)(p / plane);
  const int64_t r = p - (int64_t)*ix * plane;
  *iy = (int)(r / side);
  *iz = (int)(r - (int64_t)*iy * side);
}

// coordinate i of the grid of n steps per semi-edge
SMP_HD double smp_coordinate(int i, int n) { return (double)(i - n) * (SMP_SEMI_EDGE / (double)n); }

// cube -> homochoric ball, the operations of cubochoric_to_homochoric in its order
SMP_HD void smp_cube_to_ball(const double *xyz, double *ho) {
  const double scale = 0.8977727869612862;  // pi^(5/6) / 6^(1/6) / pi^(2/3)
  const double prek = 1.643456402972503;    // (3 pi / 4)^(1/3) 2^(1/4) / (pi^(5/6) / 6^(1/6) / 2)
  const double sr2 = 1.4142135623730951, pi = 3.141592653589793, pi_12 = 0.2617993877991494;
  const double sqrt_6_pi = 1.381976597885342, sqrt_pi = 1.7724538509055159, sqrt_24 = 4.898979485566356;
  // the axis of largest magnitude goes last (the first of equal ones, as np.argmax)
  const double a0 = fabs(xyz[0]), a1 = fabs(xyz[1]), a2 = fabs(xyz[2]);
  const int pyramid = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
  // the order (1, 2, 0), (2, 0, 1) or (0, 1, 2), by selects: no indexed array, nothing for a kernel to keep in scratch
  const double x = scale * (pyramid == 0 ? xyz[1] : pyramid == 1 ? xyz[2] : xyz[0]);
  const double y = scale * (pyramid == 0 ? xyz[2] : pyramid == 1 ? xyz[0] : xyz[1]);
  const double z = scale * (pyramid == 0 ? xyz[0] : pyramid == 1 ? xyz[1] : xyz[2]);
  double b0 = 0.0, b1 = 0.0, b2 = 0.0;
  if (fmax(fabs(x), fabs(y)) == 0.0) {
    b2 = sqrt_6_pi * z;  // on the pyramid's axis (z = 0: the cube's centre)
  } else {
    const bool flat = fabs(y) <= fabs(x);
    const double q = flat ? pi_12 * y / x : pi_12 * x / y;
    const double c = cos(q), s = sin(q);
    const double qq = (flat ? x : y) * prek / sqrt(sr2 - c);
    const double t1 = flat ? (sr2 * c - 1.0) * qq : sr2 * s * qq;
    const double t2 = flat ? sr2 * s * qq : (sr2 * c - 1.0) * qq;
    const double cc = t1 * t1 + t2 * t2;
    const double shrink = sqrt(fmax(1.0 - pi * cc / (24.0 * z * z), 0.0));
    b0 = t1 * shrink;
    b1 = t2 * shrink;
    b2 = sqrt_6_pi * z - sqrt_pi * cc / sqrt_24 / z;
  }
  ho[0] = pyramid == 0 ? b2 : pyramid == 1 ? b1 : b0;
  ho[1] = pyramid == 0 ? b0 : pyramid == 1 ? b2 : b1;
  ho[2] = pyramid == 0 ? b1 : pyramid == 1 ? b0 : b2;
}

// the rotation angle w in [0, pi] of a homochoric vector of length h: 3/4 (w - sin w) = h^3
SMP_HD double smp_angle(double h) {
  const double target = h * h * h;
  double lo = 0.0, hi = 3.141592653589793;
  for (int i = 0; i < SMP_BISECTIONS; ++i) {
    const double mid = 0.5 * (lo + hi);
    const bool below = 0.75 * (mid - sin(mid)) < target;
    lo = below ? mid : lo;
    hi = below ? hi : mid;
  }
  return 0.5 * (lo + hi);
}

// homochoric vector -> unit quaternion (q0 >= 0)
SMP_HD void smp_ball_to_quaternion(const double *ho, double *q) {
  const double h = sqrt(ho[0] * ho[0] + ho[1] * ho[1] + ho[2] * ho[2]);
  const double w = smp_angle(h);
  const double s = sin(0.5 * w);
  q[0] = cos(0.5 * w);
  q[1] = h > 0.0 ? ho[0] / h * s : 0.0;
  q[2] = h > 0.0 ? ho[1] / h * s : 0.0;
  q[3] = h > 0.0 ? ho[2] / h * s : 0.0;
}

// the quaternion of grid point p
SMP_HD void smp_point_quaternion(int64_t p, int steps, double *q) {
  int ix, iy, iz;
  smp_decode(p, 2 * steps + 1, &ix, &iy, &iz);
  const double xyz[3] = {smp_coordinate(ix, steps), smp_coordinate(iy, steps), smp_coordinate(iz, steps)};
  double ho[3];
  smp_cube_to_ball(xyz, ho);
  smp_ball_to_quaternion(ho, q);
}

// the closed face rule: both faces of every pair are kept
SMP_HD bool smp_in_zone(const double *q, const SmpFaces &faces) {
  bool keep = true;
  for (int j = 0; j < faces.n; ++j) {
    const double *f = faces.f[j];
    keep = keep && fabs(q[1] * f[0] + q[2] * f[1] + q[3] * f[2]) <= f[3] * q[0] + SMP_FACE_SLACK;
  }
  return keep;
}

}  // namespace kpdi
