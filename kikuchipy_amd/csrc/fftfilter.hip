// fftfilter.hip - FFT filter of every resident experimental pattern, in place, output in the input dtype
// (signals/ebsd.py:805-930 EBSD.fft_filter, pattern/chunk.py:75-127, pattern/_pattern.py:213-345, filters/fft_barnes.py):
//   p -> f32 -> filtered f -> rescale_intensity(f, dtype_out=<dtype>) = per-pattern min / max -> linear map onto the
//   dtype range -> .astype (truncation).
//
// Frequency domain: f = Re(ifft2(fft2(p) H')).  p is real, so f = ifft2(fft2(p) Hs) with Hs the Hermitian part of H'
// (folded on the host, pattern/_pattern.py of this package), and only the columns l = 0 ... sx/2 are transformed:
// a row DFT of length sx for those columns, a column DFT of length sy times the table Hs (scaled by 1 / (sy sx) on the
// host), an inverse column DFT, and a half-spectrum -> real inverse row DFT that counts twice every column whose mirror
// is not stored (once l = 0 and, for even sx, l = sx/2).  The DFT runs on p - mean: a constant adds Hs(0, 0) times it
// to every pixel, which the min / max rescale removes, and without it the other coefficients would carry the rounding of
// partial sums as large as the pattern's.  The DFTs (pattern_dft.h) run in f32, the rescale in f64: the reference's
// spectrum times a float64 transfer function is complex128.
//
// Spatial domain: Barnes' FFT convolution with its edge-replicating pad is a correlation with clamped indices centred
// at (ty / 2, tx / 2) (scipy.ndimage.correlate(mode="nearest")).  It is evaluated directly, the taps wave-uniform
// (scalar loads) and the sums in f64; the taps are the kernel rounded to f32 (fft_barnes.py pads it into a float32
// array) and the rescale runs in f32, as the reference's float32 result does.
//
// Degenerate patterns: a non-finite value anywhere makes the reference's FFT all NaN, and a constant filtered result
// is its 0 / 0; both give NaN before the cast.  C's cast of NaN to an integer is undefined, so the epilogue defines it:
// integer dtypes get 0 (what NumPy's astype gives on x86-64 hosts for uint8 / uint16 / int8 / int16), float dtypes NaN.
// Which path takes a shape: fftfilter_plan.h.
//
// Order of the f64 sum behind the mean, float32(sum / npix) (tests/_spectral_restate.py restates it): thread t of 256 adds,
// path 0, the quads t, t + 256, ... of four consecutive pixels each (ff_load; a short last quad padded with zeros), path 1
// the single pixels t, t + 256, ... (ff_stats_kernel); then block_reduce (pattern_dft.h).  Sums of integer patterns are
// exact, so there the two paths give the same bits; float patterns may differ in the mean's last bit.  KPDI_FFT_FILTER_PATH=1
// forces path 1, KPDI_PATTERN_BATCH=<patterns> caps a workspace batch (both read at each call, for the tests).
#include "../../include/kpdi.h"
#include "fftfilter_plan.h"
#include "kernels.h"
#include "pattern_dft.h"
#include "prep_device.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace kpdi {

namespace {

constexpr int FF_WAVES = FF_THREADS / 64;

// NaN before the cast -> 0 for integer dtypes, NaN for float dtypes; in-range values truncate as ndarray.astype
template <typename T, typename V>
__device__ __forceinline__ T ff_cast(V v) {
  if constexpr (std::is_floating_point<T>::value) return (T)v;
  else return v == v ? (T)v : (T)0;
}

// rescale_intensity's arithmetic (pattern/_pattern.py:96-111) in V = double (frequency) or float (spatial)
template <typename V>
struct FfRescale {
  V imin, irange, orange, omin;
  bool nan_case;
  __device__ __forceinline__ FfRescale(float mn, float mx, float lo, float hi, int bad) {
    imin = (V)mn;
    irange = (V)mx - (V)mn;
    orange = (V)hi - (V)lo;
    omin = (V)lo;
    nan_case = bad || !(mx > mn) || !isfinite(mx - mn);  // (all-NaN: mn = inf, mx = -inf)
  }
  template <typename T>
  __device__ __forceinline__ T operator()(float v) const {
    if (nan_case) return ff_cast<T>(__builtin_nan(""));
    return ff_cast<T>((((V)v - imin) / irange) * orange + omin);
  }
};

// the result of one pattern (`val`, f32, npix values; not read in the NaN case) -> the pattern, quads of vector stores
// where the pattern is aligned
template <typename T, typename V>
__device__ __forceinline__ void ff_store(T *__restrict__ p, const float *val, int npix, const FfRescale<V> &r, bool vec) {
  const int nquad = (npix + 3) >> 2;
  for (int q = threadIdx.x; q < nquad; q += FF_THREADS) {
    Quad<T> u;
#pragma unroll
    for (int e = 0; e < 4; ++e) u.v[e] = r.template operator()<T>(4 * q + e < npix && !r.nan_case ? val[4 * q + e] : 0.f);
    if (vec) {
      *reinterpret_cast<Quad<T> *>(p + 4 * q) = u;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < npix) p[4 * q + e] = u.v[e];
    }
  }
}

template <typename T>
__device__ __forceinline__ bool ff_vec(const T *p, int npix) {
  return (npix & 3) == 0 && ((uintptr_t)p) % (4 * sizeof(T)) == 0;
}

// the pattern as f32 into `pat`, its sum and non-finite flag per thread
template <typename T>
__device__ __forceinline__ void ff_load(const T *__restrict__ p, float *pat, int npix, bool vec, double &s, int &bad) {
  const int nquad = (npix + 3) >> 2;
  for (int q = threadIdx.x; q < nquad; q += FF_THREADS) {
    float w[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      const Quad<T> u = *reinterpret_cast<const Quad<T> *>(p + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = (float)u.v[e];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (4 * q + e < npix) w[e] = (float)p[4 * q + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pat[4 * q + e] = w[e];
      s += w[e];
      bad |= !isfinite(w[e]);
    }
  }
}

__device__ __forceinline__ float2 ff_cmul(float2 a, float2 b) {
  return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}

// spatial correlation with clamped indices at R vertically consecutive outputs (y0 .. y0 + R - 1, x) -> out[0 .. R-1];
// `pix(i)` reads pixel i.  Sums over the kernel's columns v, then its rows u, in f64; along u the R outputs share a
// sliding window of R input values, so each input is read once per column for all R outputs.  Every output gets the
// same products in the same order whatever R, so both paths agree bit for bit.  Lanes take consecutive x: unit-stride
// reads.
constexpr int FF_CORR_R = 4;
template <int R, typename Pix>
__device__ __forceinline__ void ff_correlate(Pix pix, int sy, int sx, int y0, int x, const double *__restrict__ taps,
                                             int ty, int tx, float *out) {
  double acc[R];
#pragma unroll
  for (int i = 0; i < R; ++i) acc[i] = 0.0;
  const int cy = ty / 2, cx = tx / 2;
  for (int v = 0; v < tx; ++v) {
    const int c = min(max(x + v - cx, 0), sx - 1);
    double a[R];
#pragma unroll
    for (int i = 0; i < R - 1; ++i) a[i] = (double)pix(min(max(y0 + i - cy, 0), sy - 1) * sx + c);
    for (int u = 0; u < ty; ++u) {
      a[R - 1] = (double)pix(min(max(y0 + u + R - 1 - cy, 0), sy - 1) * sx + c);
      const double w = taps[u * tx + v];  // (wave-uniform)
#pragma unroll
      for (int i = 0; i < R; ++i) acc[i] = __builtin_fma(w, a[i], acc[i]);
#pragma unroll
      for (int i = 0; i < R - 1; ++i) a[i] = a[i + 1];
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) out[i] = (float)acc[i];
}

// ---- path 0: one workgroup per pattern, everything in LDS --------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(FF_THREADS) void ff_freq_lds_kernel(T *__restrict__ pats, int sy, int sx,
                                                                const float2 *__restrict__ tw,
                                                                const float2 *__restrict__ hs, float lo, float hi) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int h = half_cols(sx), npix = sy * sx, inter = sy * h, tid = threadIdx.x;
  float *pat = (float *)smem;  // the pattern, then the filtered pattern
  float2 *X = (float2 *)(pat + ((npix + 3) & ~3));
  float2 *G = X + inter;
  float2 *twx = G + inter, *twy = twx + sx;
  double *red = (double *)(twy + sy);
  T *p = pats + (int64_t)blockIdx.x * npix;
  const bool vec = ff_vec(p, npix);
  for (int i = tid; i < sx + sy; i += FF_THREADS) twx[i] = tw[i];
  double s = 0;
  int bad = 0;
  ff_load(p, pat, npix, vec, s, bad);
  block_reduce<FF_WAVES, RedSum, RedOr>(red, s, bad);  // (its barriers also publish `pat` and the twiddles)
  if (bad) {
    ff_store(p, pat, npix, FfRescale<double>(0.f, 0.f, lo, hi, 1), vec);
    return;
  }
  const float mean = (float)(s / npix);
  for (int o = tid; o < inter; o += FF_THREADS) {
    const int y = o / h, l = o - y * h;
    const float *row = pat + y * sx;
    X[o] = row_dft([row](int x) { return row[x]; }, sx, l, mean, twx);
  }
  __syncthreads();
  for (int o = tid; o < inter; o += FF_THREADS) {
    const int k = o / h, l = o - k * h;
    G[o] = ff_cmul(col_dft<false>(X + l, h, sy, k, twy), hs[o]);
  }
  __syncthreads();
  for (int o = tid; o < inter; o += FF_THREADS) {
    const int y = o / h, l = o - y * h;
    const float2 v = col_dft<true>(G + l, h, sy, y, twy);
    const float c = column_count<float>(l, sx);
    X[o] = make_float2(c * v.x, c * v.y);
  }
  __syncthreads();
  float mn = __builtin_inff(), mx = -__builtin_inff();
  for (int i = tid; i < npix; i += FF_THREADS) {
    const int y = i / sx, x = i - y * sx;
    const float v = row_idft(X + y * h, h, sx, x, twx);
    pat[i] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  block_reduce<FF_WAVES, RedMin, RedMax>(red, mn, mx);  // (its barriers also publish `pat`)
  ff_store(p, pat, npix, FfRescale<double>(mn, mx, lo, hi, 0), vec);
}

template <typename T>
__global__ __launch_bounds__(FF_THREADS) void ff_spatial_lds_kernel(T *__restrict__ pats, int sy, int sx,
                                                                   const double *__restrict__ taps, int ty, int tx,
                                                                   float lo, float hi) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int npix = sy * sx, npix4 = (npix + 3) & ~3, tid = threadIdx.x;
  float *pat = (float *)smem;
  float *res = pat + npix4;
  double *red = (double *)(res + npix4);
  T *p = pats + (int64_t)blockIdx.x * npix;
  const bool vec = ff_vec(p, npix);
  double s = 0;
  int bad = 0;
  ff_load(p, pat, npix, vec, s, bad);
  block_reduce<FF_WAVES, RedSum, RedOr>(red, s, bad);
  if (bad) {
    ff_store(p, res, npix, FfRescale<float>(0.f, 0.f, lo, hi, 1), vec);
    return;
  }
  float mn = __builtin_inff(), mx = -__builtin_inff();
  const int jobs = (sy + FF_CORR_R - 1) / FF_CORR_R * sx;
  for (int job = tid; job < jobs; job += FF_THREADS) {
    const int yb = job / sx, x = job - yb * sx, y0 = yb * FF_CORR_R;
    float v[FF_CORR_R];
    ff_correlate<FF_CORR_R>([pat](int j) { return pat[j]; }, sy, sx, y0, x, taps, ty, tx, v);
#pragma unroll
    for (int i = 0; i < FF_CORR_R; ++i)
      if (y0 + i < sy) {
        res[(y0 + i) * sx + x] = v[i];
        mn = fminf(mn, v[i]);
        mx = fmaxf(mx, v[i]);
      }
  }
  block_reduce<FF_WAVES, RedMin, RedMax>(red, mn, mx);
  ff_store(p, res, npix, FfRescale<float>(mn, mx, lo, hi, 0), vec);
}

// ---- path 1: intermediates in a device workspace, many workgroups per pattern ------------------------------------------
// workspace of a batch of b patterns, frequency: X [b][inter] float2 | G [b][inter] float2 (the f32 result of pattern i
// at (float *)(G + i inter)) | stats [b][2] double (mean, non-finite); spatial: R [b][npix4] float | stats [b][2]
struct FfWs {
  float2 *X, *G;
  float *R;
  int64_t rstride;  // floats between the results of consecutive patterns
  double *stats;
};

template <typename T>
__global__ __launch_bounds__(FF_THREADS) void ff_stats_kernel(const T *__restrict__ pats, int npix, FfWs ws) {
  __shared__ double red[2 * FF_WAVES];
  const T *p = pats + (int64_t)blockIdx.x * npix;
  double s = 0;
  int bad = 0;
  for (int i = threadIdx.x; i < npix; i += FF_THREADS) {
    const float v = (float)p[i];
    s += v;
    bad |= !isfinite(v);
  }
  block_reduce<FF_WAVES, RedSum, RedOr>(red, s, bad);
  if (threadIdx.x == 0) {
    ws.stats[2 * blockIdx.x] = (double)(float)(s / npix);
    ws.stats[2 * blockIdx.x + 1] = bad ? 1.0 : 0.0;
  }
}

template <typename T>
__global__ __launch_bounds__(FF_THREADS) void ff_rows_kernel(const T *__restrict__ pats, int sy, int sx, int bpp,
                                                            const float2 *__restrict__ tw, FfWs ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2 *twx = (float2 *)smem;
  const int h = half_cols(sx), inter = sy * h;
  const int i = blockIdx.x / bpp, o = (blockIdx.x - i * bpp) * FF_THREADS + threadIdx.x;
  for (int j = threadIdx.x; j < sx; j += FF_THREADS) twx[j] = tw[j];
  __syncthreads();
  if (o >= inter || ws.stats[2 * i + 1] != 0.0) return;
  const float mean = (float)ws.stats[2 * i];
  const int y = o / h, l = o - y * h;
  const T *row = pats + (int64_t)i * sy * sx + (int64_t)y * sx;
  ws.X[(int64_t)i * inter + o] = row_dft([row](int x) { return (float)row[x]; }, sx, l, mean, twx);
}

// INV = false: G = DFT_col(X) * Hs; INV = true: X = count * IDFT_col(G)
template <bool INV>
__global__ __launch_bounds__(FF_THREADS) void ff_cols_kernel(int sy, int sx, int bpp, const float2 *__restrict__ tw,
                                                            const float2 *__restrict__ hs, FfWs ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2 *twy = (float2 *)smem;
  const int h = half_cols(sx), inter = sy * h;
  const int i = blockIdx.x / bpp, o = (blockIdx.x - i * bpp) * FF_THREADS + threadIdx.x;
  for (int j = threadIdx.x; j < sy; j += FF_THREADS) twy[j] = tw[sx + j];
  __syncthreads();
  if (o >= inter || ws.stats[2 * i + 1] != 0.0) return;
  const int k = o / h, l = o - k * h;
  if (!INV) {
    ws.G[(int64_t)i * inter + o] = ff_cmul(col_dft<false>(ws.X + (int64_t)i * inter + l, h, sy, k, twy), hs[o]);
  } else {
    const float2 v = col_dft<true>(ws.G + (int64_t)i * inter + l, h, sy, k, twy);
    const float c = column_count<float>(l, sx);
    ws.X[(int64_t)i * inter + o] = make_float2(c * v.x, c * v.y);
  }
}

__global__ __launch_bounds__(FF_THREADS) void ff_irows_kernel(int sy, int sx, int bpp, const float2 *__restrict__ tw,
                                                             FfWs ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2 *twx = (float2 *)smem;
  const int h = half_cols(sx), inter = sy * h, npix = sy * sx;
  const int i = blockIdx.x / bpp, o = (blockIdx.x - i * bpp) * FF_THREADS + threadIdx.x;
  for (int j = threadIdx.x; j < sx; j += FF_THREADS) twx[j] = tw[j];
  __syncthreads();
  if (o >= npix || ws.stats[2 * i + 1] != 0.0) return;
  const int y = o / sx, x = o - y * sx;
  ws.R[i * ws.rstride + o] = row_idft(ws.X + (int64_t)i * inter + (int64_t)y * h, h, sx, x, twx);
}

template <typename T>
__global__ __launch_bounds__(FF_THREADS) void ff_spatial_ws_kernel(const T *__restrict__ pats, int sy, int sx, int bpp,
                                                                  const double *__restrict__ taps, int ty, int tx,
                                                                  FfWs ws) {
  const int npix = sy * sx;
  const int i = blockIdx.x / bpp, o = (blockIdx.x - i * bpp) * FF_THREADS + threadIdx.x;
  if (o >= npix || ws.stats[2 * i + 1] != 0.0) return;
  const T *p = pats + (int64_t)i * npix;
  const int y = o / sx, x = o - y * sx;
  ff_correlate<1>([p](int j) { return (float)p[j]; }, sy, sx, y, x, taps, ty, tx, ws.R + i * ws.rstride + o);
}

// one workgroup per pattern: min / max of the result, rescale, cast, store
template <typename T, typename V>
__global__ __launch_bounds__(FF_THREADS) void ff_epilogue_kernel(T *__restrict__ pats, int npix, FfWs ws, float lo,
                                                                float hi) {
  __shared__ double red[2 * FF_WAVES];
  T *p = pats + (int64_t)blockIdx.x * npix;
  const float *r = ws.R + blockIdx.x * ws.rstride;
  const int bad = ws.stats[2 * blockIdx.x + 1] != 0.0;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  if (!bad)
    for (int i = threadIdx.x; i < npix; i += FF_THREADS) {
      mn = fminf(mn, r[i]);
      mx = fmaxf(mx, r[i]);
    }
  block_reduce<FF_WAVES, RedMin, RedMax>(red, mn, mx);
  ff_store(p, r, npix, FfRescale<V>(mn, mx, lo, hi, bad), ff_vec(p, npix));
}

template <typename T>
hipError_t launch_ff_t(const FfLaunch &a, const FfPlan &plan, hipStream_t s) {
  T *pats = (T *)a.patterns;
  const float2 *tw = (const float2 *)a.twiddles;
  const float2 *hs = (const float2 *)a.table;
  const bool freq = a.domain == FF_DOMAIN_FREQUENCY;
  if (plan.path == 0) {
    const void *k = freq ? (const void *)ff_freq_lds_kernel<T> : (const void *)ff_spatial_lds_kernel<T>;
    if (plan.lds_bytes > 64 * 1024) {
      hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
      if (e != hipSuccess) return e;
    }
    if (freq)
      hipLaunchKernelGGL(ff_freq_lds_kernel<T>, dim3((unsigned)a.n), dim3(FF_THREADS), plan.lds_bytes, s, pats, a.sy,
                         a.sx, tw, hs, a.omin, a.omax);
    else
      hipLaunchKernelGGL(ff_spatial_lds_kernel<T>, dim3((unsigned)a.n), dim3(FF_THREADS), plan.lds_bytes, s, pats, a.sy,
                         a.sx, a.taps, a.ty, a.tx, a.omin, a.omax);
    return hipGetLastError();
  }
  if (!a.workspace || a.workspace_bytes < plan.workspace_bytes) return hipErrorInvalidValue;
  const int64_t inter = (int64_t)a.sy * half_cols(a.sx), npix = (int64_t)a.sy * a.sx;
  FfWs ws;
  if (freq) {
    ws.X = (float2 *)a.workspace;
    ws.G = ws.X + plan.batch * inter;
    ws.R = (float *)ws.G;
    ws.rstride = 2 * inter;
    ws.stats = (double *)(ws.G + plan.batch * inter);
  } else {
    ws.X = ws.G = nullptr;
    ws.R = (float *)a.workspace;
    ws.rstride = (int64_t)ff_pix4(a.sy, a.sx);
    ws.stats = (double *)(ws.R + plan.batch * ws.rstride);
  }
  const size_t tw_x = (size_t)a.sx * 8, tw_y = (size_t)a.sy * 8;
  for (int64_t start = 0; start < a.n; start += plan.batch) {
    const int64_t b = std::min<int64_t>(plan.batch, a.n - start);
    T *p = pats + start * npix;
    hipLaunchKernelGGL(ff_stats_kernel<T>, dim3((unsigned)b), dim3(FF_THREADS), 0, s, p, (int)npix, ws);
    if (freq) {
      const int bh = plan.blocks_half, bp = plan.blocks_pix;
      hipLaunchKernelGGL(ff_rows_kernel<T>, dim3((unsigned)(b * bh)), dim3(FF_THREADS), tw_x, s, p, a.sy, a.sx, bh, tw, ws);
      hipLaunchKernelGGL(ff_cols_kernel<false>, dim3((unsigned)(b * bh)), dim3(FF_THREADS), tw_y, s, a.sy, a.sx, bh, tw, hs,
                         ws);
      hipLaunchKernelGGL(ff_cols_kernel<true>, dim3((unsigned)(b * bh)), dim3(FF_THREADS), tw_y, s, a.sy, a.sx, bh, tw, hs,
                         ws);
      hipLaunchKernelGGL(ff_irows_kernel, dim3((unsigned)(b * bp)), dim3(FF_THREADS), tw_x, s, a.sy, a.sx, bp, tw, ws);
      hipLaunchKernelGGL((ff_epilogue_kernel<T, double>), dim3((unsigned)b), dim3(FF_THREADS), 0, s, p, (int)npix, ws,
                         a.omin, a.omax);
    } else {
      const int bp = plan.blocks_pix;
      hipLaunchKernelGGL(ff_spatial_ws_kernel<T>, dim3((unsigned)(b * bp)), dim3(FF_THREADS), 0, s, p, a.sy, a.sx, bp,
                         a.taps, a.ty, a.tx, ws);
      hipLaunchKernelGGL((ff_epilogue_kernel<T, float>), dim3((unsigned)b), dim3(FF_THREADS), 0, s, p, (int)npix, ws,
                         a.omin, a.omax);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

FfPlan fft_filter_launch_plan(int domain, int sy, int sx, int64_t n) {
  bool force = false;
  int64_t cap = 0;
  if (const char *e = getenv("KPDI_FFT_FILTER_PATH")) force = atoi(e) == 1;  // tests: path 1 for any shape
  if (const char *e = getenv("KPDI_PATTERN_BATCH")) cap = atoll(e) > 0 ? atoll(e) : 0;  // tests: several batches
  return ff_plan(domain, sy, sx, n, force, cap);
}

hipError_t launch_fft_filter(const FfLaunch &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const FfPlan plan = fft_filter_launch_plan(a.domain, a.sy, a.sx, a.n);
  if (plan.path < 0 || (plan.path == 0 && a.n >= (int64_t)INT32_MAX) ||
      (plan.path == 1 && plan.batch * std::max(plan.blocks_half, plan.blocks_pix) >= (int64_t)INT32_MAX))
    return hipErrorInvalidValue;
  if (a.domain == FF_DOMAIN_FREQUENCY ? (!a.table || !a.twiddles) : (!a.taps || a.ty < 1 || a.tx < 1))
    return hipErrorInvalidValue;
  return with_pattern_type(a.dtype, [&](auto t) { return launch_ff_t<decltype(t)>(a, plan, s); });
}

}  // namespace kpdi
