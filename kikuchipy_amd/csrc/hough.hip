// hough.hip - Hough indexing (kikuchipy_amd/indexing/_hough_indexing.py): the Radon transform of the
// resident patterns, band detection in the sinograms, and indexing of the bands.  What a sinogram cell, a band and a
// pattern's vote compute is in hough_plan.h and hough_vote.h, the same C++ a host test compiles.  No atomics; every sum
// runs in a fixed order; every output is written by exactly one thread.
//
//   radon: one workgroup per pattern, any of the six pattern dtypes -> f32.  Thread t sums the masked pixels t, t + 256, ...
//          in float64, thread 0 adds the 256 partial sums in order: the masked mean.  The staged pattern (mask applied,
//          mean removed) goes to LDS when it fits (hough_plan), else to the pattern's slot of the workspace; then one
//          thread per sinogram cell walks its line.
//   bands: one workgroup per pattern: smoothing along rho, then along theta across the seam, the local maxima, and
//          n_bands rounds of a workgroup arg-max under a total order (value, then cell index) - order-independent.
//   index: one thread per pattern and phase (hough_vote.h), float64; the phase's tables staged in LDS.
//   pc search: one lane per pattern runs that pattern's Nelder-Mead search over the projection centre around the same
//          vote (hough_search.h), a bounded number of evaluations per launch; the searches rest in device memory.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "hough_plan.h"
#include "hough_vote.h"
#include "hough_search.h"

namespace kpdi {

namespace {

template <typename T, bool LDS>
__global__ __launch_bounds__(HOUGH_THREADS) void hough_radon_kernel(const T *patterns, HoughGeom g, const float *cos_sin,
                                                                   float *workspace, size_t pattern_floats) {
  extern __shared__ __attribute__((aligned(16))) unsigned char hough_lds[];
  double *partial = reinterpret_cast<double *>(hough_lds);
  float *ws = workspace + (size_t)blockIdx.x * pattern_floats;
  float *staged = LDS ? reinterpret_cast<float *>(hough_lds + HOUGH_LDS_SCRATCH) : ws + 3 * (size_t)g.n_theta * g.n_rho;
  const T *p = patterns + (size_t)blockIdx.x * g.ny * g.nx;
  const int npix = g.ny * g.nx;
  double sum = 0.0;
  for (int o = threadIdx.x; o < npix; o += HOUGH_THREADS)
    if (hough_in_mask(g, o / g.nx, o % g.nx)) sum += (double)p[o];
  partial[threadIdx.x] = sum;
  __syncthreads();
  double total = 0.0;
  for (int t = 0; t < HOUGH_THREADS; ++t) total += partial[t];  // (every thread: the same order, the same bits)
  const float mean = (float)(total / (double)g.n_mask);
  for (int o = threadIdx.x; o < npix; o += HOUGH_THREADS)
    staged[o] = hough_in_mask(g, o / g.nx, o % g.nx) ? (float)p[o] - mean : 0.0f;
  __syncthreads();
  const int cells = g.n_theta * g.n_rho;
  for (int o = threadIdx.x; o < cells; o += HOUGH_THREADS) {
    const int a = o / g.n_rho, k = o - a * g.n_rho;
    ws[o] = hough_line_sum(staged, g, cos_sin[a], cos_sin[g.n_theta + a], k);
  }
}

__global__ __launch_bounds__(HOUGH_THREADS) void hough_bands_kernel(HoughGeom g, HoughSmooth w, int n_bands, float *workspace,
                                                                   size_t pattern_floats, HoughBand *bands) {
  __shared__ float best_v[HOUGH_THREADS];
  __shared__ int best_i[HOUGH_THREADS];
  const int cells = g.n_theta * g.n_rho;
  float *s = workspace + (size_t)blockIdx.x * pattern_floats, *tmp = s + cells, *u = tmp + cells;
  for (int o = threadIdx.x; o < cells; o += HOUGH_THREADS) tmp[o] = hough_smooth_rho(s, g, w, o / g.n_rho, o % g.n_rho);
  __syncthreads();
  for (int o = threadIdx.x; o < cells; o += HOUGH_THREADS) u[o] = hough_smooth_theta(tmp, g, w, o / g.n_rho, o % g.n_rho);
  __syncthreads();
  // tmp: the value at a peak, -inf elsewhere
  for (int o = threadIdx.x; o < cells; o += HOUGH_THREADS)
    tmp[o] = hough_is_peak(u, g, w, o / g.n_rho, o % g.n_rho) ? u[o] : -INFINITY;
  __syncthreads();
  HoughBand *out = bands + (size_t)blockIdx.x * n_bands;
  float last_v = INFINITY;
  int last_i = -1;
  for (int b = 0; b < n_bands; ++b) {
    // the first peak, in the order of hough_before, that comes after the one taken last
    float v = -INFINITY;
    int at = -1;
    for (int o = threadIdx.x; o < cells; o += HOUGH_THREADS) {
      const float c = tmp[o];
      if (c == -INFINITY || !hough_before(last_v, last_i, c, o)) continue;
      if (at < 0 || hough_before(c, o, v, at)) {
        v = c;
        at = o;
      }
    }
    best_v[threadIdx.x] = v;
    best_i[threadIdx.x] = at;
    __syncthreads();
    for (int half = HOUGH_THREADS / 2; half > 0; half >>= 1) {
      if ((int)threadIdx.x < half) {
        const float v2 = best_v[threadIdx.x + half];
        const int i2 = best_i[threadIdx.x + half];
        if (i2 >= 0 && (best_i[threadIdx.x] < 0 || hough_before(v2, i2, best_v[threadIdx.x], best_i[threadIdx.x]))) {
          best_v[threadIdx.x] = v2;
          best_i[threadIdx.x] = i2;
        }
      }
      __syncthreads();
    }
    last_v = best_v[0];
    last_i = best_i[0];
    __syncthreads();  // (read before the next round writes)
    if (last_i < 0) {  // no peak is left: this band and the rest are empty (every thread takes this branch)
      if (threadIdx.x == 0)
        for (int e = b; e < n_bands; ++e) out[e] = HoughBand{0.0f, 0.0f, 0.0f, 0, -1, -1, 0.0f, 0.0f};
      break;
    }
    if (threadIdx.x == 0) out[b] = hough_band_at(u, g, last_i / g.n_rho, last_i % g.n_rho);
  }
}

struct IndexArgs {
  const HoughBand *bands;  // [m][n_bands]
  int64_t m;
  int n_bands;
  const double *pcs;       // [n_pc][3], n_pc = 1 or m
  int64_t n_pc;
  HvDetector det;
  HvPhase phase;
  double *quat, *fit, *cm;  // [m][4], [m], [m]
  int32_t *nmatch;          // [m]
};

// dynamic LDS of the index kernel: the phase's angles, normals and families, read many times by every thread
size_t index_lds_bytes(int n) { return (size_t)n * n * 8 + (size_t)n * 3 * 8 + (size_t)n * 4; }

__global__ __launch_bounds__(64) void hough_index_kernel(IndexArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char index_lds[];
  const int P = a.phase.n;
  double *angles = reinterpret_cast<double *>(index_lds), *refl = angles + (size_t)P * P;
  int32_t *family = reinterpret_cast<int32_t *>(refl + 3 * (size_t)P);
  for (int o = threadIdx.x; o < P * P; o += 64) angles[o] = a.phase.angles[o];
  for (int o = threadIdx.x; o < 3 * P; o += 64) refl[o] = a.phase.normals[o];
  for (int o = threadIdx.x; o < P; o += 64) family[o] = a.phase.family[o];
  __syncthreads();
  a.phase.angles = angles;
  a.phase.normals = refl;
  a.phase.family = family;
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= a.m) return;
  const double *pc = a.pcs + 3 * (a.n_pc == 1 ? 0 : i);
  double normals[HV_MAX_BANDS][3];
  int nb = 0;
  for (int b = 0; b < a.n_bands; ++b) {
    const HoughBand band = a.bands[i * a.n_bands + b];
    if (band.valid && hv_band_normal((double)band.theta, (double)band.rho, pc, a.det.ny, a.det.nx, normals[nb])) ++nb;
  }
  const HvResult r = hv_index(normals, nb, a.n_bands, a.phase, a.det);
  for (int k = 0; k < 4; ++k) a.quat[4 * i + k] = r.quat[k];
  a.fit[i] = r.fit;
  a.cm[i] = r.cm;
  a.nmatch[i] = r.indexed ? r.nmatch : 0;
}

// One lane per pattern advances that pattern's search by at most `evals` evaluations; the searches live in `states`
// between launches.  Every lane walks the same bounded loop (hv_pc_search_advance), one that is done idling
// through it, so a wave diverges inside the vote and not around it.  done[i]: 1 once search i has ended.
__global__ __launch_bounds__(HOUGH_SEARCH_MAX_LANES) void hough_pc_search_kernel(HoughPcSearchLaunch a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char index_lds[];
  const int P = a.phase.n, lanes = (int)blockDim.x;
  double *angles = reinterpret_cast<double *>(index_lds), *refl = angles + (size_t)P * P;
  int32_t *family = reinterpret_cast<int32_t *>(refl + 3 * (size_t)P);
  for (int o = threadIdx.x; o < P * P; o += lanes) angles[o] = a.phase.angles[o];
  for (int o = threadIdx.x; o < 3 * P; o += lanes) refl[o] = a.phase.normals[o];
  for (int o = threadIdx.x; o < P; o += lanes) family[o] = a.phase.family[o];
  __syncthreads();
  a.phase.angles = angles;
  a.phase.normals = refl;
  a.phase.family = family;
  const int64_t i = (int64_t)blockIdx.x * lanes + threadIdx.x;
  if (i >= a.m) return;
  HoughPcSearch s = a.states[i];
  const bool done = hv_pc_search_advance(s, a.bands + i * a.n_bands, a.n_bands, a.det, a.phase, a.options, a.evals);
  a.states[i] = s;
  a.done[i] = done ? 1 : 0;
}

// pc, fun, nfev, nit and status of the finished searches
__global__ __launch_bounds__(64) void hough_pc_search_result_kernel(const HoughPcSearch *states, int64_t m, double *pc, double *fun,
                                                                   int32_t *nfev, int32_t *nit, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= m) return;
  const HoughPcSearch &s = states[i];
  for (int k = 0; k < 3; ++k) pc[3 * i + k] = s.nm.sim[0][k];
  fun[i] = s.nm.fun();
  nfev[i] = s.nm.fcalls;
  nit[i] = s.nm.iterations;
  status[i] = hv_pc_search_status(s);
}

template <typename T>
hipError_t launch_radon_t(const HoughBandsLaunch &l, hipStream_t s) {
  const size_t floats = l.plan.pattern_bytes / sizeof(float);
  if (l.plan.lds) {
    if (l.plan.lds_bytes > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute((const void *)hough_radon_kernel<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)l.plan.lds_bytes);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((hough_radon_kernel<T, true>), dim3((unsigned)l.n), dim3(HOUGH_THREADS), l.plan.lds_bytes, s,
                       (const T *)l.patterns, l.geom, l.cos_sin, l.workspace, floats);
  } else {
    hipLaunchKernelGGL((hough_radon_kernel<T, false>), dim3((unsigned)l.n), dim3(HOUGH_THREADS), l.plan.lds_bytes, s,
                       (const T *)l.patterns, l.geom, l.cos_sin, l.workspace, floats);
  }
  return hipGetLastError();
}

}  // namespace

// the sinograms of `l.n` patterns (one pass) into the first third of each pattern's workspace slot
hipError_t launch_hough_radon(const HoughBandsLaunch &l, hipStream_t s) {
  if (!l.patterns || !l.cos_sin || !l.workspace || l.n < 1 || l.n > 2147483647LL || !l.plan.ok) return hipErrorInvalidValue;
  return with_pattern_type(l.dtype, [&](auto t) { return launch_radon_t<decltype(t)>(l, s); });
}

// the bands of the sinograms launch_hough_radon left in the workspace
hipError_t launch_hough_bands(const HoughBandsLaunch &l, hipStream_t s) {
  if (!l.workspace || !l.bands || l.n < 1 || l.n > 2147483647LL || l.n_bands < 1 || l.n_bands > HOUGH_MAX_BANDS ||
      l.smooth.rim < 1 || 2 * l.smooth.rim >= l.geom.n_rho || l.smooth.rt < 0 || l.smooth.rr < 0 ||
      2 * l.smooth.rt + 1 > HOUGH_MAX_TAPS || 2 * l.smooth.rr + 1 > HOUGH_MAX_TAPS || l.smooth.rt > l.geom.n_theta)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hough_bands_kernel, dim3((unsigned)l.n), dim3(HOUGH_THREADS), 0, s, l.geom, l.smooth, l.n_bands, l.workspace,
                     l.plan.pattern_bytes / sizeof(float), l.bands);
  return hipGetLastError();
}

hipError_t launch_hough_index(const HoughBand *bands, int64_t m, int n_bands, const double *pcs, int64_t n_pc, const HvDetector &det,
                              const HvPhase &phase, double *quat, double *fit, double *cm, int32_t *nmatch, hipStream_t s) {
  if (!bands || !pcs || !quat || !fit || !cm || !nmatch || m < 1 || (m + 63) / 64 > 2147483647LL || n_bands < 1 ||
      n_bands > HV_MAX_BANDS || (n_pc != 1 && n_pc != m) || phase.n < 1 || phase.n > HV_MAX_REFLECTORS || phase.n_families < 1 ||
      phase.n_families > HV_MAX_FAMILIES)
    return hipErrorInvalidValue;
  IndexArgs a{bands, m, n_bands, pcs, n_pc, det, phase, quat, fit, cm, nmatch};
  const size_t lds = index_lds_bytes(phase.n);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)hough_index_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(hough_index_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), lds, s, a);
  return hipGetLastError();
}

// one launch of the projection-centre searches: every search that is not done advances by at most l.evals evaluations
hipError_t launch_hough_pc_search(const HoughPcSearchLaunch &l, const HoughSearchPlan &plan, hipStream_t s) {
  if (!l.bands || !l.states || !l.done || l.m < 1 || !plan.ok || plan.lanes < 1 || plan.lanes > HOUGH_SEARCH_MAX_LANES ||
      plan.workgroups != (l.m + plan.lanes - 1) / plan.lanes || l.n_bands < 1 || l.n_bands > HV_MAX_BANDS || l.evals < 1 ||
      l.phase.n < 1 || l.phase.n > HV_MAX_REFLECTORS || l.phase.n_families < 1 || l.phase.n_families > HV_MAX_FAMILIES ||
      l.options.maxiter < 1 || l.options.maxfun < 1)
    return hipErrorInvalidValue;
  const size_t lds = index_lds_bytes(l.phase.n);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)hough_pc_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(hough_pc_search_kernel, dim3((unsigned)plan.workgroups), dim3((unsigned)plan.lanes), lds, s, l);
  return hipGetLastError();
}

hipError_t launch_hough_pc_search_results(const HoughPcSearch *states, int64_t m, double *pc, double *fun, int32_t *nfev,
                                          int32_t *nit, int32_t *status, hipStream_t s) {
  if (!states || !pc || !fun || !nfev || !nit || !status || m < 1 || (m + 63) / 64 > 2147483647LL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hough_pc_search_result_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, states, m, pc, fun, nfev, nit,
                     status);
  return hipGetLastError();
}

}  // namespace kpdi
