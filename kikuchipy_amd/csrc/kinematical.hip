// kinematical.hip - the kinematical master pattern in the stereographic projection
// (KikuchiPatternSimulator.calculate_master_pattern, simulations/kikuchi_pattern_simulator.py:162-199; get_pattern,
// :685-700), with the reference's arithmetic as plain Python evaluates it.  For the direction v of a pixel and every
// reflector i (unit normal u, theta1 = pi/2 - theta, intensity I), in rising i, in float64:
//
//   D = ((u0 v0) + u1 v1) + u2 v2           (vec_dot, _utils/numba.py:88; no contraction: -ffp-contract=off)
//   |D| <= 1e-7:                            pattern += 0.5 I
//   else angle = acos(D); theta1 <= angle <= pi/2:   pattern += I       (D > 1: NaN, nothing; D < 0: nothing)
//
// One thread per pixel, blockIdx.y the hemisphere (the lower hemisphere's direction is the upper one's with z negated,
// exactly -pole * z of the reference).  The reflector table is staged in LDS a chunk at a time; every lane reads the
// same entry, a broadcast.  acos is evaluated only for pairs inside the screen of kinematical_plan.h: pairs outside it
// fall on the same side of the band test whatever acos rounds to.  No atomics, vector stores
// only, one summation order per pixel: the result does not depend on the chunk length or the launch, bit for bit.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "kinematical_plan.h"

#include <cmath>
#include <cstdlib>

namespace kpdi {

namespace {

struct KinArgs {
  const double *dirs;   // [pixels][3], upper hemisphere
  const double *table;  // [m][KIN_ENTRY_DOUBLES]
  double *out;          // [grid_y][pixels]
  int pixels, m, chunk;
  double zsign0, zsign1;
};

__global__ __launch_bounds__(KIN_THREADS) void kinematical_master_pattern_kernel(KinArgs a) {
  __shared__ __attribute__((aligned(16))) double tab[KIN_CHUNK * KIN_ENTRY_DOUBLES];
  const int pix = blockIdx.x * KIN_THREADS + threadIdx.x;
  const bool live = pix < a.pixels;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;
  if (live) {
    const double *d = a.dirs + (size_t)pix * 3;
    v0 = d[0];
    v1 = d[1];
    v2 = d[2] * (blockIdx.y ? a.zsign1 : a.zsign0);
  }
  const double half_pi = 1.5707963267948966;  // np.pi / 2
  double sum = 0.0;
  for (int base = 0; base < a.m; base += a.chunk) {
    const int len = a.m - base < a.chunk ? a.m - base : a.chunk;
    __syncthreads();  // the previous chunk has been read by every lane
    const double2 *src = reinterpret_cast<const double2 *>(a.table + (size_t)base * KIN_ENTRY_DOUBLES);
    for (int i = threadIdx.x; i < len * (KIN_ENTRY_DOUBLES / 2); i += KIN_THREADS) reinterpret_cast<double2 *>(tab)[i] = src[i];
    __syncthreads();
    for (int j = 0; j < len; ++j) {
      const double *e = tab + j * KIN_ENTRY_DOUBLES;
      const double D = ((e[0] * v0) + e[1] * v1) + e[2] * v2;
      if (fabs(D) <= KIN_HALF_WIDTH) {
        sum += 0.5 * e[3];
      } else if (D > 0.0) {
        // (D < 0: acos(D) > pi/2 + 1e-7, outside)
        if (D <= e[4]) {
          sum += e[3];
        } else if (!(D >= e[5])) {
          const double angle = acos(D);
          if (angle <= half_pi && angle >= e[6]) sum += e[3];
        }
      }
    }
  }
  if (live) a.out[(size_t)blockIdx.y * a.pixels + pix] = sum;
}

}  // namespace

KinPlan kinematical_launch_plan(int64_t m, int half_size, int hemispheres) {
  int force = 0;
  if (const char *e = getenv("KPDI_KINEMATICAL_CHUNK")) force = atoi(e);  // tests: chunk boundaries at small reflector counts
  return kin_plan(m, half_size, hemispheres, force);
}

hipError_t launch_kinematical_master_pattern(const KinLaunch &l, hipStream_t s) {
  const KinPlan plan = kinematical_launch_plan(l.m, l.half_size, l.hemispheres);
  if (!plan.ok || !l.dirs || !l.table || !l.out) return hipErrorInvalidValue;
  KinArgs a{};
  a.dirs = l.dirs;
  a.table = l.table;
  a.out = l.out;
  a.pixels = (int)plan.pixels;
  a.m = (int)l.m;
  a.chunk = plan.chunk;
  a.zsign0 = kin_zsign(l.hemispheres, 0);
  a.zsign1 = kin_zsign(l.hemispheres, 1);
  hipLaunchKernelGGL(kinematical_master_pattern_kernel, dim3((unsigned)plan.grid_x, (unsigned)plan.grid_y), dim3(KIN_THREADS), 0,
                     s, a);
  return hipGetLastError();
}

}  // namespace kpdi
