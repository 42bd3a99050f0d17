// iq.hip - image quality (Krieger Lassen's Q) of every resident experimental pattern
// (pattern/_pattern.py:698-775 get_image_quality, :365-386 fft_frequency_vectors, :349-362 fft_spectrum):
//   p -> f32 -> (normalize) p - mean -> F = DFT2(p) -> S = |F| -> Q = 1 - (sum S w / sum S) / inertia_max.
// Q is invariant under scaling p, so the reference's division by std changes rounding only and is not done here; its
// one visible effect, 0/0 for a constant pattern, is kept as an exact test (minimum == maximum: NaN).  A non-finite
// value anywhere gives NaN, as the reference's arithmetic does.  The DFT always runs on p - mean: a constant changes
// F(0, 0) alone, so without `normalize` |F(0, 0)| is the pattern's f64 sum instead, and the other coefficients do not
// carry the rounding of partial sums as large as the whole pattern's.
//
// Half-spectrum DFT (pattern_dft.h): p is real, so |F(k, l)| = |F(-k, -l)|.  The host folds the weights
// (W(k, l) = w(k, l) + w(-k, -l) for the columns whose mirror is not computed, else w(k, l)) and the count c(l) (2 or 1)
// is applied to S here, so inertia = sum W S / sum c S is the full-spectrum sum exactly.  Sums of the DFT run in f32,
// per-pattern statistics and the weighted sums in f64.
// Which path takes a shape: iq_plan.h.
//
// Order of the f64 sums (tests/_spectral_restate.py restates it).  The pattern's sum, on both paths: thread t of 256 adds
// the pixels t, t + 256, ... in turn, then block_reduce (pattern_dft.h).  The two weighted sums: path 0, thread t adds the
// terms of the coefficients t, t + 256, ... in turn, then block_reduce; path 1, one term per thread, block_reduce per
// workgroup of 256 coefficients (iq_cols_kernel), then the workgroups in order from 0 (iq_final_kernel).
// KPDI_IQ_PATH=1 forces path 1, KPDI_PATTERN_BATCH=<patterns> caps a workspace batch (both read at each call, for the tests).
#include "../../include/kpdi.h"
#include "iq_plan.h"
#include "kernels.h"
#include "pattern_dft.h"

#include <cstdlib>

namespace kpdi {

namespace {

constexpr int IQ_WAVES = IQ_THREADS / 64;

template <typename T>
__device__ __forceinline__ float as_f32(T v) { return (float)v; }

// the value, the pattern statistics of one thread's pixels
template <typename T>
__device__ __forceinline__ void stat_one(T raw, double &s, float &lo, float &hi, int &bad) {
  const float v = as_f32(raw);
  s += v;
  lo = fminf(lo, v);
  hi = fmaxf(hi, v);
  bad |= !isfinite(v);
}

// |F(k, l)| of the intermediate column `col` (pattern_dft.h)
__device__ __forceinline__ float col_dft_abs(const float2 *col, int h, int sy, int k, const float2 *tw) {
  const float2 f = col_dft<false>(col, h, sy, k, tw);
  return sqrtf(f.x * f.x + f.y * f.y);
}

// ---- path 0: one workgroup per pattern, everything in LDS ----------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(IQ_THREADS) void iq_lds_kernel(const T *__restrict__ pats, int sy, int sx, int normalize,
                                                           const float2 *__restrict__ tw, const double *__restrict__ wfold,
                                                           double inertia_max, float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int h = half_cols(sx), npix = sy * sx, inter = sy * h, tid = threadIdx.x;
  float2 *X = (float2 *)smem;
  float2 *twx = X + inter, *twy = twx + sx;
  double *red = (double *)(twy + sy);
  float *pat = (float *)(red + 4 * IQ_WAVES);
  const T *p = pats + (int64_t)blockIdx.x * npix;
  for (int i = tid; i < sx + sy; i += IQ_THREADS) twx[i] = tw[i];
  double s = 0;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  int bad = 0;
  for (int i = tid; i < npix; i += IQ_THREADS) {
    stat_one(p[i], s, lo, hi, bad);
    pat[i] = as_f32(p[i]);
  }
  block_reduce<IQ_WAVES, RedSum, RedMin, RedMax, RedOr>(red, s, lo, hi, bad);  // (its barriers also publish `pat` and the twiddles)
  if (bad || (normalize && lo == hi)) {
    if (tid == 0) out[blockIdx.x] = __builtin_nanf("");
    return;
  }
  const float mean = (float)(s / npix);
  for (int o = tid; o < inter; o += IQ_THREADS) {
    const int y = o / h, l = o - y * h;
    const float *row = pat + y * sx;
    X[o] = row_dft([row](int x) { return row[x]; }, sx, l, mean, twx);
  }
  __syncthreads();
  double sw = 0, ss = 0;
  for (int o = tid; o < inter; o += IQ_THREADS) {
    const int k = o / h, l = o - k * h;
    const float f = col_dft_abs(X + l, h, sy, k, twy);
    const double a = (o == 0 && !normalize) ? fabs(s) : (double)f;
    sw += wfold[o] * a;
    ss += column_count<double>(l, sx) * a;
  }
  block_reduce<IQ_WAVES, RedSum, RedSum>(red, sw, ss);
  if (tid == 0) out[blockIdx.x] = (float)(1.0 - (sw / ss) / inertia_max);
}

// ---- path 1: the intermediate in a device workspace, many workgroups per pattern ----------------------------------------
// workspace of a batch of b patterns: X [b][sy * h] float2 | stats [b][3] double (mean, degenerate, sum) |
// partial [b][bpp][2]
struct IqWs {
  float2 *X;
  double *stats, *partial;
};

template <typename T>
__global__ __launch_bounds__(IQ_THREADS) void iq_stats_kernel(const T *__restrict__ pats, int npix, int normalize, IqWs ws) {
  __shared__ double red[4 * IQ_WAVES];
  const T *p = pats + (int64_t)blockIdx.x * npix;
  double s = 0;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  int bad = 0;
  for (int i = threadIdx.x; i < npix; i += IQ_THREADS) stat_one(p[i], s, lo, hi, bad);
  block_reduce<IQ_WAVES, RedSum, RedMin, RedMax, RedOr>(red, s, lo, hi, bad);
  if (threadIdx.x == 0) {
    ws.stats[3 * blockIdx.x] = (double)(float)(s / npix);
    ws.stats[3 * blockIdx.x + 1] = (bad || (normalize && lo == hi)) ? 1.0 : 0.0;
    ws.stats[3 * blockIdx.x + 2] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(IQ_THREADS) void iq_rows_kernel(const T *__restrict__ pats, int sy, int sx, int bpp,
                                                            const float2 *__restrict__ tw, IqWs ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2 *twx = (float2 *)smem;
  const int h = half_cols(sx), inter = sy * h;
  const int i = blockIdx.x / bpp, o = (blockIdx.x - i * bpp) * IQ_THREADS + threadIdx.x;
  for (int j = threadIdx.x; j < sx; j += IQ_THREADS) twx[j] = tw[j];
  __syncthreads();
  if (o >= inter || ws.stats[3 * i + 1] != 0.0) return;
  const float mean = (float)ws.stats[3 * i];
  const int y = o / h, l = o - y * h;
  const T *row = pats + (int64_t)i * sy * sx + (int64_t)y * sx;
  ws.X[(int64_t)i * inter + o] = row_dft([row](int x) { return as_f32(row[x]); }, sx, l, mean, twx);
}

__global__ __launch_bounds__(IQ_THREADS) void iq_cols_kernel(int sy, int sx, int bpp, int normalize, const float2 *__restrict__ tw,
                                                            const double *__restrict__ wfold, IqWs ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2 *twy = (float2 *)smem;
  double *red = (double *)(twy + sy);
  const int h = half_cols(sx), inter = sy * h;
  const int i = blockIdx.x / bpp, b = blockIdx.x - i * bpp, o = b * IQ_THREADS + threadIdx.x;
  for (int j = threadIdx.x; j < sy; j += IQ_THREADS) twy[j] = tw[sx + j];
  __syncthreads();
  if (ws.stats[3 * i + 1] != 0.0) return;  // uniform over the workgroup
  double sw = 0, ss = 0;
  if (o < inter) {
    const int k = o / h, l = o - k * h;
    const float f = col_dft_abs(ws.X + (int64_t)i * inter + l, h, sy, k, twy);
    const double a = (o == 0 && !normalize) ? fabs(ws.stats[3 * i + 2]) : (double)f;
    sw = wfold[o] * a;
    ss = column_count<double>(l, sx) * a;
  }
  block_reduce<IQ_WAVES, RedSum, RedSum>(red, sw, ss);
  if (threadIdx.x == 0) {
    ws.partial[2 * ((int64_t)i * bpp + b)] = sw;
    ws.partial[2 * ((int64_t)i * bpp + b) + 1] = ss;
  }
}

__global__ void iq_final_kernel(int64_t n, int bpp, double inertia_max, IqWs ws, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (ws.stats[3 * i + 1] != 0.0) {
    out[i] = __builtin_nanf("");
    return;
  }
  double sw = 0, ss = 0;
  for (int b = 0; b < bpp; ++b) {
    sw += ws.partial[2 * (i * bpp + b)];
    ss += ws.partial[2 * (i * bpp + b) + 1];
  }
  out[i] = (float)(1.0 - (sw / ss) / inertia_max);
}

template <typename T>
hipError_t launch_iq_t(const IqLaunch &a, const IqPlan &plan, hipStream_t s) {
  const T *pats = (const T *)a.patterns;
  const float2 *tw = (const float2 *)a.twiddles;
  if (plan.path == 0) {
    if (plan.lds_bytes > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute((const void *)iq_lds_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)plan.lds_bytes);
      if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(iq_lds_kernel<T>, dim3((unsigned)a.n), dim3(IQ_THREADS), plan.lds_bytes, s, pats, a.sy, a.sx,
                       a.normalize, tw, a.wfold, a.inertia_max, a.out);
    return hipGetLastError();
  }
  if (!a.workspace || a.workspace_bytes < plan.workspace_bytes) return hipErrorInvalidValue;
  const int64_t inter = (int64_t)a.sy * half_cols(a.sx), npix = (int64_t)a.sy * a.sx;
  const int bpp = plan.blocks_per_pattern;
  IqWs ws;
  ws.X = (float2 *)a.workspace;
  ws.stats = (double *)(ws.X + plan.batch * inter);
  ws.partial = ws.stats + 3 * plan.batch;
  for (int64_t start = 0; start < a.n; start += plan.batch) {
    const int64_t b = std::min<int64_t>(plan.batch, a.n - start);
    const T *p = pats + start * npix;
    hipLaunchKernelGGL(iq_stats_kernel<T>, dim3((unsigned)b), dim3(IQ_THREADS), 0, s, p, (int)npix, a.normalize, ws);
    hipLaunchKernelGGL(iq_rows_kernel<T>, dim3((unsigned)(b * bpp)), dim3(IQ_THREADS), (size_t)a.sx * 8, s, p, a.sy, a.sx,
                       bpp, tw, ws);
    hipLaunchKernelGGL(iq_cols_kernel, dim3((unsigned)(b * bpp)), dim3(IQ_THREADS),
                       (size_t)a.sy * 8 + 2 * IQ_WAVES * 8, s, a.sy, a.sx, bpp, a.normalize, tw, a.wfold, ws);
    hipLaunchKernelGGL(iq_final_kernel, dim3((unsigned)((b + 255) / 256)), dim3(256), 0, s, b, bpp, a.inertia_max, ws,
                       a.out + start);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

IqPlan image_quality_launch_plan(int sy, int sx, int64_t n) {
  bool force = false;
  int64_t cap = 0;
  if (const char *e = getenv("KPDI_IQ_PATH")) force = atoi(e) == 1;  // tests: path 1 for any shape
  if (const char *e = getenv("KPDI_PATTERN_BATCH")) cap = atoll(e) > 0 ? atoll(e) : 0;  // tests: several batches
  return iq_plan(sy, sx, n, force, cap);
}

hipError_t launch_image_quality(const IqLaunch &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const IqPlan plan = image_quality_launch_plan(a.sy, a.sx, a.n);
  if (plan.path < 0 || (plan.path == 0 && a.n >= (int64_t)INT32_MAX) ||
      (plan.path == 1 && plan.batch * plan.blocks_per_pattern >= (int64_t)INT32_MAX))
    return hipErrorInvalidValue;
  return with_pattern_type(a.dtype, [&](auto t) { return launch_iq_t<decltype(t)>(a, plan, s); });
}

}  // namespace kpdi
