// neighbours.hip - the two ops whose output at a map point depends on the patterns around it:
//
// Neighbour pattern averaging (EBSD.average_neighbour_patterns, signals/ebsd.py:943-1111; pattern/chunk.py:130-164), as
// NumPy evaluates the reference (scipy.ndimage.correlate, then the rescale), per map point q:
//   1. c = float32(sum_j w_j float32(p_{q+j})): the window offsets j in C order, zero coefficients and points outside
//      the map left out (they add an exact 0), accumulated in float64 and rounded once;
//   2. a = float64(c) / float64(ws_q), ws_q the integer window sum of the point (the caller's, of the WHOLE map);
//   3. r = (a - min a) / (max a - min a) * (omax - omin) + omin in float64, cast to the data dtype by truncation
//      (integer dtypes) or rounding (float dtypes).  min / max are taken on c (float32, exactly reducible) and divided
//      by ws_q afterwards: the division is monotonic.  A NaN in c makes the whole pattern NaN, as np.min does; a constant
//      averaged pattern is 0 / 0, i.e. 0 for integer dtypes and NaN for float dtypes, as in intensity.hip.
// The stencil reads its neighbours' ORIGINAL values, so it writes a second buffer (the caller swaps it in).
//
// Neighbour dot products (EBSD.get_neighbour_dot_product_matrices / get_average_neighbour_dot_product_map,
// signals/ebsd.py:1221-1491; signals/util/_map_helper.py): a statistics pass (mean, sum (x - mean)^2 of every resident
// pattern) and a pass with one workgroup per map point that holds the centred centre pattern and streams its
// neighbours: dp[q, j] = sum (x_q - m_q) (x_{q+j} - m_{q+j}) / (n_q n_{q+j}), everything in float64 in a fixed order.
// n = 0 gives 0 / 0 = NaN (a constant pattern under zero_mean + normalize) and a NaN in a pattern reaches its mean and
// hence every product it takes part in, as in the reference.  The map is the mean of the point's non-NaN products.
//
// Both are memory-bound stencils over whole patterns; nothing depends on scheduling (no atomics), so a map split by
// rows over several contexts gives the bits of one context.  Layout: neighbours_plan.h.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "neighbours_plan.h"
#include "pattern_dft.h"
#include "prep_device.h"

#include <cmath>
#include <type_traits>

namespace kpdi {

namespace {

constexpr int NB_WAVES = NB_THREADS / 64;

// VEC consecutive values of a pattern from item `item` on
template <typename T, int VEC>
__device__ __forceinline__ void nb_load(const T *p, int item, T v[VEC]) {
  if constexpr (VEC == 4) {
    const Quad<T> u = *reinterpret_cast<const Quad<T> *>(p + 4 * (size_t)item);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = u.v[e];
  } else {
    v[0] = p[item];
  }
}

// ndarray.astype(TO) / the assignment cast of a float64 result
template <typename TO>
__device__ __forceinline__ TO nb_cast(double y) {
  if constexpr (std::is_floating_point<TO>::value) {
    return (TO)y;
  } else {
    const int32_t i = (y >= -2147483648.0 && y < 2147483648.0) ? (int32_t)y : INT32_MIN;  // NaN: INT32_MIN
    return (TO)(uint32_t)i;
  }
}

__device__ __forceinline__ bool nb_inside(int y, int x, int ny, int nx) { return y >= 0 && y < ny && x >= 0 && x < nx; }

// step 1 of the averaging for one item of the point (y, x)
template <typename T, int VEC>
__device__ __forceinline__ void nb_correlate(const NbAvgLaunch &a, const T *src, int npix, int y, int x, int item,
                                             float c[VEC]) {
  double acc[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
  for (int t = 0; t < a.ntaps; ++t) {
    const NbTap tap = a.taps[t];
    const int yy = y + tap.dy, xx = x + tap.dx;
    if (!nb_inside(yy, xx, a.ny, a.nx)) continue;
    T v[VEC];
    nb_load<T, VEC>(src + ((int64_t)yy * a.nx + xx) * npix, item, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] += (double)(float)v[e] * tap.w;
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) c[e] = (float)acc[e];
}

template <typename T, int VEC>
__device__ __forceinline__ void nb_store(T *dst, int item, const float c[VEC], double ws, double imin, double span,
                                         double orange, double omin) {
  T r[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) r[e] = nb_cast<T>((((double)c[e] / ws - imin) / span) * orange + omin);
  if constexpr (VEC == 4) {
    Quad<T> u;
#pragma unroll
    for (int e = 0; e < 4; ++e) u.v[e] = r[e];
    *reinterpret_cast<Quad<T> *>(dst + 4 * (size_t)item) = u;
  } else {
    dst[item] = r[0];
  }
}

template <int VEC>
__device__ __forceinline__ void nb_range(const float c[VEC], float &mn, float &mx, int &nan) {
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    mn = fminf(mn, c[e]);
    mx = fmaxf(mx, c[e]);
    nan |= c[e] != c[e];
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(NB_THREADS) void nb_average_kernel(NbAvgLaunch a) {
  __shared__ double red[3 * NB_WAVES];
  const int npix = a.sy * a.sx, nitem = npix / VEC, tid = threadIdx.x;
  const int64_t pt = (int64_t)a.row0 * a.nx + blockIdx.x;
  const int y = (int)(pt / a.nx), x = (int)(pt % a.nx);
  const T *src = (const T *)a.src;
  T *dst = (T *)a.dst + pt * npix;
  const double ws = a.ws[pt];
  constexpr int KEEP_ITEMS = NB_KEEP / VEC;
  const bool keep = nitem <= NB_THREADS * KEEP_ITEMS;
  float c[NB_KEEP];
  float mn = __builtin_inff(), mx = -__builtin_inff();
  int nan = 0;
  if (keep) {
#pragma unroll
    for (int k = 0; k < KEEP_ITEMS; ++k) {
      const int item = tid + k * NB_THREADS;
      if (item < nitem) {
        nb_correlate<T, VEC>(a, src, npix, y, x, item, c + k * VEC);
        nb_range<VEC>(c + k * VEC, mn, mx, nan);
      }
    }
  } else {
    for (int item = tid; item < nitem; item += NB_THREADS) {
      nb_correlate<T, VEC>(a, src, npix, y, x, item, c);
      nb_range<VEC>(c, mn, mx, nan);
    }
  }
  block_reduce<NB_WAVES, RedMin, RedMax, RedOr>(red, mn, mx, nan);
  double imin = (double)(ws > 0 ? mn : mx) / ws, imax = (double)(ws > 0 ? mx : mn) / ws;
  if (nan) imin = imax = __builtin_nan("");
  const double span = imax - imin;
  if (keep) {
#pragma unroll
    for (int k = 0; k < KEEP_ITEMS; ++k) {
      const int item = tid + k * NB_THREADS;
      if (item < nitem) nb_store<T, VEC>(dst, item, c + k * VEC, ws, imin, span, a.orange, a.omin);
    }
  } else {
    for (int item = tid; item < nitem; item += NB_THREADS) {
      nb_correlate<T, VEC>(a, src, npix, y, x, item, c);
      nb_store<T, VEC>(dst, item, c, ws, imin, span, a.orange, a.omin);
    }
  }
}

// stats[p] = (mean of pattern p, or 0 without zero_mean; sum (x - mean)^2)
template <typename T, int VEC>
__global__ __launch_bounds__(NB_THREADS) void nb_stats_kernel(const T *src, int npix, int zero_mean, double2 *stats) {
  __shared__ double red[NB_WAVES];
  const int nitem = npix / VEC, tid = threadIdx.x;
  const T *p = src + (int64_t)blockIdx.x * npix;
  double mean = 0.0;
  if (zero_mean) {
    double s = 0.0;
    for (int item = tid; item < nitem; item += NB_THREADS) {
      T v[VEC];
      nb_load<T, VEC>(p, item, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) s += (double)v[e];
    }
    block_reduce<NB_WAVES, RedSum>(red, s);
    mean = s / (double)npix;
  }
  double ss = 0.0;
  for (int item = tid; item < nitem; item += NB_THREADS) {
    T v[VEC];
    nb_load<T, VEC>(p, item, v);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const double d = (double)v[e] - mean;
      ss += d * d;
    }
  }
  block_reduce<NB_WAVES, RedSum>(red, ss);
  if (tid == 0) stats[blockIdx.x] = make_double2(mean, ss);
}

__device__ __forceinline__ void nb_put(void *out, int f64, int64_t i, double v) {
  if (f64) ((double *)out)[i] = v;
  else ((float *)out)[i] = (float)v;
}

template <typename T, int VEC>
__global__ __launch_bounds__(NB_THREADS) void nb_dot_kernel(NbDotLaunch a) {
  __shared__ double red[NB_WAVES];
  const int npix = a.sy * a.sx, nitem = npix / VEC, tid = threadIdx.x;
  const int64_t pt = (int64_t)a.row0 * a.nx + blockIdx.x, o = blockIdx.x;
  const int y = (int)(pt / a.nx), x = (int)(pt % a.nx);
  const T *src = (const T *)a.src;
  const T *pc = src + pt * npix;
  const double2 sc = a.stats[pt];
  const double na = sqrt(sc.y);
  const double nanv = __builtin_nan("");
  // every entry starts as NaN; the lane that owns an entry (j mod NB_THREADS) is also the one that fills it in later
  if (a.matrices)
    for (int j = tid; j < a.wsize; j += NB_THREADS) nb_put(a.matrices, a.f64, o * a.wsize + j, nanv);
  if (a.matrices && tid == a.jorigin % NB_THREADS)
    nb_put(a.matrices, a.f64, o * a.wsize + a.jorigin, a.normalize ? sc.y / (na * na) : sc.y);
  constexpr int KEEP_ITEMS = NB_KEEP / VEC;
  const bool keep = nitem <= NB_THREADS * KEEP_ITEMS;
  double cx[NB_KEEP];
  if (keep && a.ntaps > 0) {
#pragma unroll
    for (int k = 0; k < KEEP_ITEMS; ++k) {
      const int item = tid + k * NB_THREADS;
      T v[VEC];
      if (item < nitem) nb_load<T, VEC>(pc, item, v);
#pragma unroll
      for (int e = 0; e < VEC; ++e) cx[k * VEC + e] = item < nitem ? (double)v[e] - sc.x : 0.0;
    }
  }
  double sum = 0.0;
  int cnt = 0;
  for (int t = 0; t < a.ntaps; ++t) {
    const NbTap tap = a.taps[t];
    const int yy = y + tap.dy, xx = x + tap.dx;
    if (!nb_inside(yy, xx, a.ny, a.nx)) continue;
    const int64_t nb = (int64_t)yy * a.nx + xx;
    const T *pn = src + nb * npix;
    const double2 sn = a.stats[nb];
    double acc = 0.0;
    if (keep) {
#pragma unroll
      for (int k = 0; k < KEEP_ITEMS; ++k) {
        const int item = tid + k * NB_THREADS;
        if (item < nitem) {
          T v[VEC];
          nb_load<T, VEC>(pn, item, v);
#pragma unroll
          for (int e = 0; e < VEC; ++e) acc += cx[k * VEC + e] * ((double)v[e] - sn.x);
        }
      }
    } else {
      for (int item = tid; item < nitem; item += NB_THREADS) {
        T v[VEC], u[VEC];
        nb_load<T, VEC>(pn, item, v);
        nb_load<T, VEC>(pc, item, u);
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc += ((double)u[e] - sc.x) * ((double)v[e] - sn.x);
      }
    }
    block_reduce<NB_WAVES, RedSum>(red, acc);
    const double dp = a.normalize ? acc / (na * sqrt(sn.y)) : acc;
    if (a.matrices && tid == tap.j % NB_THREADS) nb_put(a.matrices, a.f64, o * a.wsize + tap.j, dp);
    if (dp == dp) {
      sum += dp;
      ++cnt;
    }
  }
  if (a.map && tid == 0) nb_put(a.map, a.f64, o, cnt ? sum / (double)cnt : nanv);
}

}  // namespace

hipError_t launch_neighbour_average(const NbAvgLaunch &a, hipStream_t s) {
  if (!a.src || !a.dst || !a.taps || !a.ws || a.sy < 1 || a.sx < 1 || a.ny < 1 || a.nx < 1 || a.row0 < 0 ||
      a.row1 > a.ny || a.row0 >= a.row1 || a.ntaps < 0)
    return hipErrorInvalidValue;
  const int64_t blocks = (int64_t)(a.row1 - a.row0) * a.nx;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const NbPlan pl = nb_plan(a.sy, a.sx);
  return with_pattern_type(a.dtype, [&](auto t) {
    using T = decltype(t);
    if (pl.vec == 4)
      hipLaunchKernelGGL((nb_average_kernel<T, 4>), dim3((unsigned)blocks), dim3(NB_THREADS), 0, s, a);
    else
      hipLaunchKernelGGL((nb_average_kernel<T, 1>), dim3((unsigned)blocks), dim3(NB_THREADS), 0, s, a);
    return hipGetLastError();
  });
}

hipError_t launch_neighbour_stats(const void *src, int dtype, int64_t n, int sy, int sx, int zero_mean, double *stats,
                                  hipStream_t s) {
  if (!src || !stats || n < 1 || n > 0x7fffffff || sy < 1 || sx < 1) return hipErrorInvalidValue;
  const NbPlan pl = nb_plan(sy, sx);
  const int npix = sy * sx;
  return with_pattern_type(dtype, [&](auto t) {
    using T = decltype(t);
    if (pl.vec == 4)
      hipLaunchKernelGGL((nb_stats_kernel<T, 4>), dim3((unsigned)n), dim3(NB_THREADS), 0, s, (const T *)src, npix,
                         zero_mean, (double2 *)stats);
    else
      hipLaunchKernelGGL((nb_stats_kernel<T, 1>), dim3((unsigned)n), dim3(NB_THREADS), 0, s, (const T *)src, npix,
                         zero_mean, (double2 *)stats);
    return hipGetLastError();
  });
}

hipError_t launch_neighbour_dot(const NbDotLaunch &a, hipStream_t s) {
  if (!a.src || !a.stats || (a.ntaps > 0 && !a.taps) || (!a.matrices && !a.map) || a.sy < 1 || a.sx < 1 || a.ny < 1 ||
      a.nx < 1 || a.row0 < 0 || a.row1 > a.ny || a.row0 >= a.row1 || a.ntaps < 0 || a.wsize < 1 || a.jorigin < 0 ||
      a.jorigin >= a.wsize)
    return hipErrorInvalidValue;
  const int64_t blocks = (int64_t)(a.row1 - a.row0) * a.nx;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const NbPlan pl = nb_plan(a.sy, a.sx);
  return with_pattern_type(a.dtype, [&](auto t) {
    using T = decltype(t);
    if (pl.vec == 4)
      hipLaunchKernelGGL((nb_dot_kernel<T, 4>), dim3((unsigned)blocks), dim3(NB_THREADS), 0, s, a);
    else
      hipLaunchKernelGGL((nb_dot_kernel<T, 1>), dim3((unsigned)blocks), dim3(NB_THREADS), 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace kpdi
