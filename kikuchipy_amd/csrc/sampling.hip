// sampling.hip - cubochoric sampling of a rotation group's fundamental zone (get_sample_fundamental of
// kikuchipy_amd/sampling.py; Rosca, Morawiec & De Graef 2014; Singh & De Graef 2016), in float64.  What one grid point
// computes and the launch arithmetic are in sampling_plan.h, the same C++ a host test compiles.
//
// The kept orientations leave in lexicographic grid order (x slowest), the host sampler's order, without atomics:
//   1. count: a workgroup owns SMP_THREADS consecutive points, one per thread; each wave counts its kept lanes with a
//      ballot, the workgroup's sum goes to counts[workgroup];
//   2. scan:  one workgroup turns the counts into exclusive 64-bit offsets (and the total after them), SMP_SCAN_THREADS
//      counts per round: a shuffle scan in every wave, the wave sums through LDS, the carry in a register;
//   3. emit:  the SAME kernel as 1 with an output pointer: it recomputes its point (cheaper than 32 B stored for every
//      rejected point) and a kept lane writes at offsets[workgroup] + kept lanes of the waves before it (LDS) + kept
//      lanes before it in its wave (ballot, popcount), as two 16-byte vector stores.
// One kernel for both passes: the two passes cannot disagree on a flag.  A store is also bounded by the total the scan
// found, so no arithmetic can make it leave the output.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "sampling_plan.h"

namespace kpdi {

namespace {

struct SmpArgs {
  SmpFaces faces;
  int steps;
  int64_t points;
  uint32_t *counts;        // [blocks], written by the count pass
  const int64_t *offsets;  // [blocks] exclusive, read by the emit pass
  double *out;             // [kept][4]; nullptr: the count pass
  int64_t kept;            // rows of `out`
};

__global__ __launch_bounds__(SMP_THREADS) void sampling_pass_kernel(SmpArgs a) {
  __shared__ unsigned wave_kept[SMP_WAVES];
  const int64_t p = (int64_t)blockIdx.x * SMP_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  bool keep = false;
  if (p < a.points) {
    smp_point_quaternion(p, a.steps, q);
    keep = smp_in_zone(q, a.faces);
  }
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) wave_kept[wave] = (unsigned)__popcll(mask);
  __syncthreads();
  if (!a.out) {
    if (threadIdx.x == 0) {
      unsigned sum = 0;
      for (int w = 0; w < SMP_WAVES; ++w) sum += wave_kept[w];
      a.counts[blockIdx.x] = sum;
    }
    return;
  }
  if (keep) {
    unsigned before = (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += wave_kept[w];
    const int64_t row = a.offsets[blockIdx.x] + before;
    if (row < a.kept) {
      double2 *dst = reinterpret_cast<double2 *>(a.out + row * 4);
      dst[0] = make_double2(q[0], q[1]);
      dst[1] = make_double2(q[2], q[3]);
    }
  }
}

// exclusive scan of counts[0, blocks) into offsets[0, blocks), the total into offsets[blocks]; one workgroup
__global__ __launch_bounds__(SMP_SCAN_THREADS) void sampling_scan_kernel(const uint32_t *counts, int64_t *offsets, int64_t blocks) {
  constexpr int WAVES = SMP_SCAN_THREADS / 64;
  __shared__ long long wave_sum[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long carry = 0;
  for (int64_t base = 0; base < blocks; base += SMP_SCAN_THREADS) {
    const int64_t i = base + threadIdx.x;
    const long long v = i < blocks ? (long long)counts[i] : 0;
    long long x = v;  // inclusive within the wave
    for (int d = 1; d < 64; d <<= 1) {
      const long long y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    long long before = 0, round = 0;
    for (int w = 0; w < WAVES; ++w) {
      const long long s = wave_sum[w];
      before += w < wave ? s : 0;
      round += s;
    }
    if (i < blocks) offsets[i] = carry + before + x - v;
    carry += round;
    __syncthreads();  // wave_sum is rewritten in the next round
  }
  if (threadIdx.x == 0) offsets[blocks] = carry;
}

SmpArgs pass_args(const SmpLaunch &l, const SmpPlan &plan) {
  SmpArgs a{};
  a.faces = l.faces;
  a.steps = plan.steps;
  a.points = plan.points;
  a.counts = l.counts;
  a.offsets = l.offsets;
  return a;
}

bool launch_refused(const SmpLaunch &l, const SmpPlan &plan) {
  return !plan.ok || l.faces.n < 0 || l.faces.n > SMP_MAX_FACES || !l.counts || !l.offsets;
}

}  // namespace

hipError_t launch_sampling_count(const SmpLaunch &l, hipStream_t s) {
  const SmpPlan plan = smp_plan(l.steps);
  if (launch_refused(l, plan)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sampling_pass_kernel, dim3((unsigned)plan.blocks), dim3(SMP_THREADS), 0, s, pass_args(l, plan));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sampling_scan_kernel, dim3(1), dim3(SMP_SCAN_THREADS), 0, s, l.counts, l.offsets, plan.blocks);
  return hipGetLastError();
}

hipError_t launch_sampling_emit(const SmpLaunch &l, hipStream_t s) {
  const SmpPlan plan = smp_plan(l.steps);
  if (launch_refused(l, plan) || !l.out || l.kept < 1) return hipErrorInvalidValue;
  SmpArgs a = pass_args(l, plan);
  a.out = l.out;
  a.kept = l.kept;
  hipLaunchKernelGGL(sampling_pass_kernel, dim3((unsigned)plan.blocks), dim3(SMP_THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace kpdi
