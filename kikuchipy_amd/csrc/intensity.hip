// intensity.hip - intensity rescaling and normalization of every resident experimental pattern
// (signals/_kikuchipy_signal.py:88-338 rescale_intensity / normalize_intensity, pattern/_pattern.py:31-111, :154-210),
// with the reference's arithmetic under NumPy 1.26 dtype rules:
//
//   rescale:   [np.clip(p, imin, imax)] -> ((p - imin) / float(imax - imin)) * (omax - omin) + omin -> .astype(dtype_out)
//              imin / imax: the pattern's nanmin / nanmax (INT_MODE_MINMAX), in_range (INT_MODE_RANGE: given, or the
//              global min / max of `relative`), or np.nanpercentile(p, percentiles) (INT_MODE_PERCENTILE).
//   normalize: (p - mean) / (num_std * std [* sqrt(size)]) -> .astype(dtype_out)
//
// Arithmetic dtype V: float64 for integer and float64 patterns, float32 for float32 patterns (NumPy 1.26 keeps a float32
// array float32 against Python / NumPy float64 scalars, which are rounded to float32 first).  Integer patterns are
// rescaled exactly in float64: the reference computes p - imin and imax - imin in the input's integer dtype, which wraps
// for int8 / int16 patterns whose range exceeds the type's positive range; here it does not.  For
// float32 patterns `float(imax - imin)` is the float64 difference rounded to float32 (in_range / percentiles are float64
// scalars there) or the float32 difference (nanmin / nanmax are float32 scalars); the operation order is the
// reference's and the library builds with -ffp-contract=off.
//
// Percentiles restate numpy 1.26's nanpercentile (linear method) on the order statistics: q / 100, the virtual index
// (n - 1) q in float64 with n the non-NaN count, floor and next index (both n - 1 at or above the last index, where the
// weight is the index + 1), and _lerp's two branches a + d t and b - d (1 - t) for t >= 0.5, with d = b - a in the
// pattern's dtype and the rest in float64.  The up to four order statistics come from one radix select on
// order-preserving unsigned keys (8-bit digits: 1 pass for 8-bit dtypes, 2 for 16-bit, 4 for float32, 8 for float64;
// NaN keys are not counted): the first pass builds one 256-bin LDS histogram of all keys, the later ones one per order
// statistic over the keys that share its prefix, and wave r scans histogram r.  LDS atomics only count, so the result
// does not depend on scheduling.
//
// Normalize sums in float64 (exact for integer patterns' means), in a fixed order: thread t takes the quads t, t + 256,
// ..., then a fixed shuffle / LDS tree.  For float32 patterns mean and std are rounded to float32 and
// num_std * std * sqrt(size) is formed in float64 and rounded to float32, as NumPy 1.26's scalar rules do.
//
// Casts to integer dtypes follow ndarray.astype on x86-64: truncate to int32 (NaN and values outside int32 give
// INT32_MIN), then keep the low 8 or 16 bits; casts to float32 round to nearest.
// Which path takes a shape: intensity_plan.h.
#include "../../include/kpdi.h"
#include "intensity_plan.h"
#include "kernels.h"
#include "prep_device.h"

#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace kpdi {

namespace {

constexpr int INT_WAVES = INT_THREADS / 64;

template <typename T>
struct Arith { using V = double; };
template <>
struct Arith<float> { using V = float; };

// order-preserving unsigned keys
template <typename T>
struct KeyOf;
template <>
struct KeyOf<uint8_t> {
  using K = uint32_t;
  static constexpr int bits = 8;
  __device__ static K key(uint8_t v) { return v; }
  __device__ static uint8_t value(K k) { return (uint8_t)k; }
};
template <>
struct KeyOf<int8_t> {
  using K = uint32_t;
  static constexpr int bits = 8;
  __device__ static K key(int8_t v) { return (uint8_t)v ^ 0x80u; }
  __device__ static int8_t value(K k) { return (int8_t)(uint8_t)(k ^ 0x80u); }
};
template <>
struct KeyOf<uint16_t> {
  using K = uint32_t;
  static constexpr int bits = 16;
  __device__ static K key(uint16_t v) { return v; }
  __device__ static uint16_t value(K k) { return (uint16_t)k; }
};
template <>
struct KeyOf<int16_t> {
  using K = uint32_t;
  static constexpr int bits = 16;
  __device__ static K key(int16_t v) { return (uint16_t)v ^ 0x8000u; }
  __device__ static int16_t value(K k) { return (int16_t)(uint16_t)(k ^ 0x8000u); }
};
template <>
struct KeyOf<float> {
  using K = uint32_t;
  static constexpr int bits = 32;
  __device__ static K key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
  }
  __device__ static float value(K k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }
};
template <>
struct KeyOf<double> {
  using K = uint64_t;
  static constexpr int bits = 64;
  __device__ static K key(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  }
  __device__ static double value(K k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
  }
};

template <typename T>
__device__ __forceinline__ bool int_isnan(T v) {
  if constexpr (std::is_floating_point<T>::value) return v != v;
  else return false;
}

// block-wide reduction with `op`, a fixed tree (xor shuffles, then the waves in order); every thread gets the result
template <typename Op>
__device__ __forceinline__ double int_block_reduce(double v, double *red, Op op) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  __syncthreads();  // `red` may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
  for (int i = 1; i < INT_WAVES; ++i) r = op(r, red[i]);
  return r;
}
struct OpSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };  // NaN-ignoring
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// quad q of a pattern (LDS or global): the number of valid values
template <typename T>
__device__ __forceinline__ int int_load4(const T *p, int npix, int q, bool vec, T v[4]) {
  if (vec) {
    const Quad<T> u = *reinterpret_cast<const Quad<T> *>(p + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = u.v[e];
    return 4;
  }
  const int m = npix - 4 * q < 4 ? npix - 4 * q : 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = e < m ? p[4 * q + e] : T(0);
  return m;
}

// np.maximum / np.minimum (NaN-propagating), as np.clip = minimum(maximum(p, lo), hi)
template <typename V>
__device__ __forceinline__ V int_clip(V x, V lo, V hi) {
  x = (x > lo || x != x) ? x : lo;
  return (x < hi || x != x) ? x : hi;
}

template <typename V>
struct IntMap {
  bool normalize, clip;
  V lo, hi, imin, range, orange, omin;  // rescale
  V mean, den;                          // normalize
  __device__ __forceinline__ V operator()(V x) const {
    if (normalize) return (x - mean) / den;
    if (clip) x = int_clip(x, lo, hi);
    return ((x - imin) / range) * orange + omin;
  }
};

template <typename T, typename TO, typename V>
__device__ __forceinline__ void int_store(const T *p, TO *__restrict__ o, int npix, int nquad, bool vec,
                                          const IntMap<V> &m) {
  for (int q = threadIdx.x; q < nquad; q += INT_THREADS) {
    T v[4];
    const int c = int_load4(p, npix, q, vec, v);
    Quad<TO> u;
#pragma unroll
    for (int e = 0; e < 4; ++e) u.v[e] = astype_cast<TO>(m((V)v[e]));
    if (vec) {
      *reinterpret_cast<Quad<TO> *>(o + 4 * q) = u;
    } else {
      for (int e = 0; e < c; ++e) o[4 * q + e] = u.v[e];
    }
  }
}

// the keys of ranks rank[0..3] among the non-NaN values of the pattern (radix select, 8-bit digits)
template <typename T>
__device__ __forceinline__ void int_select(const T *p, int npix, int nquad, bool vec, const int64_t rank[4],
                                           typename KeyOf<T>::K key_out[4], unsigned (*hist)[256],
                                           typename KeyOf<T>::K *s_prefix, unsigned *s_k) {
  using KT = KeyOf<T>;
  using K = typename KT::K;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  if (tid < 4) {
    s_prefix[tid] = 0;
    s_k[tid] = (unsigned)rank[tid];
  }
  for (int shift = KT::bits - 8; shift >= 0; shift -= 8) {
    const bool first = shift == KT::bits - 8;
    for (int i = tid; i < 4 * 256; i += INT_THREADS) hist[i >> 8][i & 255] = 0;
    __syncthreads();
    K pre[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pre[r] = s_prefix[r];
    for (int q = tid; q < nquad; q += INT_THREADS) {
      T v[4];
      const int c = int_load4(p, npix, q, vec, v);
      for (int e = 0; e < c; ++e) {
        if (int_isnan(v[e])) continue;
        const K k = KT::key(v[e]);
        const unsigned d = (unsigned)(k >> shift) & 255u;
        if (first) {
          atomicAdd(&hist[0][d], 1u);
        } else {
          const K hi = k >> (shift + 8);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (hi == pre[r]) atomicAdd(&hist[r][d], 1u);
        }
      }
    }
    __syncthreads();
    // wave w: the digit of order statistic w
    const unsigned *h = hist[first ? 0 : w];
    unsigned c[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      c[j] = h[4 * lane + j];
      s += c[j];
    }
    unsigned incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    const unsigned excl = incl - s, k = s_k[w];
    if (excl <= k && k < incl) {
      unsigned acc = excl;
      int j = 0;
      while (j < 3 && k >= acc + c[j]) acc += c[j++];
      s_prefix[w] = (K)((s_prefix[w] << 8) | (K)(4 * lane + j));
      s_k[w] = k - acc;
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) key_out[r] = s_prefix[r];
}

// numpy 1.26 _quantile, linear method, for one q: the two ranks and the weight
__device__ __forceinline__ void int_quantile_index(double q, int64_t n, int64_t &prev, int64_t &next, double &t) {
  const double vi = (double)(n - 1) * q;
  if (vi >= (double)(n - 1)) {  // index -1: the last value; the weight is taken against -1
    prev = next = n - 1;
    t = vi - (-1.0);
  } else if (vi < 0) {
    prev = next = 0;
    t = vi;
  } else {
    const double f = floor(vi);
    prev = (int64_t)f;
    next = prev + 1;
    t = vi - f;
  }
}

// _lerp(a, b, t): d = b - a in the pattern's dtype (exact for the integer dtypes), the rest in float64
template <typename T>
__device__ __forceinline__ double int_lerp(T a, T b, double t) {
  double d;
  if constexpr (std::is_same<T, float>::value) d = (double)(b - a);
  else d = (double)b - (double)a;
  return t >= 0.5 ? (double)b - d * (1.0 - t) : (double)a + d * t;
}

template <typename T, bool STAGED>
__global__ __launch_bounds__(INT_THREADS) void intensity_kernel(IntLaunch a) {
  using V = typename Arith<T>::V;
  using K = typename KeyOf<T>::K;
  extern __shared__ __attribute__((aligned(32))) unsigned char int_lds[];
  __shared__ double red[INT_WAVES];
  __shared__ unsigned hist[4][256];
  __shared__ K s_prefix[4];
  __shared__ unsigned s_k[4];
  const int npix = a.sy * a.sx;
  const int64_t pat = blockIdx.x;
  const T *p = (const T *)a.src + pat * npix;
  if constexpr (STAGED) {
    // the pattern's bytes into LDS: 16-byte words where the pattern's size allows them (its start is then aligned)
    const size_t bytes = (size_t)npix * sizeof(T);
    const unsigned char *g = (const unsigned char *)p;
    if ((bytes & 15) == 0) {
      for (size_t i = threadIdx.x; i < bytes / 16; i += INT_THREADS)
        reinterpret_cast<uint4 *>(int_lds)[i] = reinterpret_cast<const uint4 *>(g)[i];
    } else if ((bytes & 3) == 0) {
      for (size_t i = threadIdx.x; i < bytes / 4; i += INT_THREADS)
        reinterpret_cast<uint32_t *>(int_lds)[i] = reinterpret_cast<const uint32_t *>(g)[i];
    } else {
      for (size_t i = threadIdx.x; i < bytes; i += INT_THREADS) int_lds[i] = g[i];
    }
    __syncthreads();
    p = (const T *)int_lds;
  }
  const int nquad = (npix + 3) >> 2;
  const bool vec = (npix & 3) == 0;
  const double dnan = __builtin_nan("");

  IntMap<V> m{};
  m.orange = (V)a.orange;
  m.omin = (V)a.omin;
  if (a.mode == INT_MODE_NORMALIZE) {
    double s = 0;
    for (int q = threadIdx.x; q < nquad; q += INT_THREADS) {
      T v[4];
      const int c = int_load4(p, npix, q, vec, v);
      for (int e = 0; e < c; ++e) s += (double)v[e];
    }
    const double mean = int_block_reduce(s, red, OpSum()) / (double)npix;
    double ss = 0;
    for (int q = threadIdx.x; q < nquad; q += INT_THREADS) {
      T v[4];
      const int c = int_load4(p, npix, q, vec, v);
      for (int e = 0; e < c; ++e) {
        const double d = (double)v[e] - mean;
        ss += d * d;
      }
    }
    const double sd = sqrt(int_block_reduce(ss, red, OpSum()) / (double)npix);
    m.normalize = true;
    m.mean = (V)mean;
    double den = a.num_std * (double)(V)sd;  // num_std * std: a float64 scalar (std is float32 for float32 patterns)
    if (a.divide_by_square_root) den = den * sqrt((double)npix);
    m.den = (V)den;
  } else {
    m.normalize = false;
    double lo, hi;  // imin, imax
    if (a.mode == INT_MODE_MINMAX) {
      double mn = dnan, mx = dnan;  // nanmin / nanmax: NaN only for an all-NaN pattern
      for (int q = threadIdx.x; q < nquad; q += INT_THREADS) {
        T v[4];
        const int c = int_load4(p, npix, q, vec, v);
        for (int e = 0; e < c; ++e) {
          mn = fmin(mn, (double)v[e]);
          mx = fmax(mx, (double)v[e]);
        }
      }
      lo = int_block_reduce(mn, red, OpMin());
      hi = int_block_reduce(mx, red, OpMax());
      m.clip = false;
      m.imin = (V)lo;
      // float(imax - imin): the float32 difference of float32 scalars, else float64 (exact for integer patterns)
      if constexpr (std::is_same<V, float>::value) m.range = (float)hi - (float)lo;
      else m.range = hi - lo;
    } else {
      if (a.mode == INT_MODE_RANGE) {
        lo = a.lo;
        hi = a.hi;
      } else {  // INT_MODE_PERCENTILE
        int64_t n = npix;
        if constexpr (std::is_floating_point<T>::value) {
          double cnt = 0;
          for (int q = threadIdx.x; q < nquad; q += INT_THREADS) {
            T v[4];
            const int c = int_load4(p, npix, q, vec, v);
            for (int e = 0; e < c; ++e) cnt += int_isnan(v[e]) ? 0.0 : 1.0;
          }
          n = (int64_t)int_block_reduce(cnt, red, OpSum());
        }
        if (n == 0) {  // all NaN: nanpercentile gives NaN
          lo = hi = dnan;
        } else {
          int64_t rank[4];
          double t0, t1;
          int_quantile_index(a.q0, n, rank[0], rank[1], t0);
          int_quantile_index(a.q1, n, rank[2], rank[3], t1);
          K keys[4];
          int_select<T>(p, npix, nquad, vec, rank, keys, hist, s_prefix, s_k);
          lo = int_lerp(KeyOf<T>::value(keys[0]), KeyOf<T>::value(keys[1]), t0);
          hi = int_lerp(KeyOf<T>::value(keys[2]), KeyOf<T>::value(keys[3]), t1);
        }
      }
      m.clip = true;
      m.lo = (V)lo;
      m.hi = (V)hi;
      m.imin = (V)lo;
      m.range = (V)(hi - lo);  // float(imax - imin) of float64 scalars
    }
  }
  const int64_t off = pat * npix;
  switch (a.dtype_out) {
    case KPDI_U8: int_store(p, (uint8_t *)a.dst + off, npix, nquad, vec, m); break;
    case KPDI_I8: int_store(p, (int8_t *)a.dst + off, npix, nquad, vec, m); break;
    case KPDI_U16: int_store(p, (uint16_t *)a.dst + off, npix, nquad, vec, m); break;
    case KPDI_I16: int_store(p, (int16_t *)a.dst + off, npix, nquad, vec, m); break;
    case KPDI_F32: int_store(p, (float *)a.dst + off, npix, nquad, vec, m); break;
    case KPDI_F64: int_store(p, (double *)a.dst + off, npix, nquad, vec, m); break;
    default: break;
  }
}

// kpdi_intensity_range: per block min / max (NaN-ignoring) and a NaN flag, then one block combines them in order
template <typename T>
__global__ __launch_bounds__(INT_THREADS) void int_range_partial_kernel(const T *__restrict__ src, int64_t count,
                                                                        double *partial) {
  __shared__ double red[INT_WAVES];
  const double dnan = __builtin_nan("");
  double mn = dnan, mx = dnan, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * INT_THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * INT_THREADS) {
    const double v = (double)src[i];
    if (v != v) bad = 1;
    mn = fmin(mn, v);
    mx = fmax(mx, v);
  }
  mn = int_block_reduce(mn, red, OpMin());
  mx = int_block_reduce(mx, red, OpMax());
  bad = int_block_reduce(bad, red, OpMax());
  if (threadIdx.x == 0) {
    partial[3 * blockIdx.x] = mn;
    partial[3 * blockIdx.x + 1] = mx;
    partial[3 * blockIdx.x + 2] = bad;
  }
}

__global__ __launch_bounds__(INT_THREADS) void int_range_final_kernel(const double *partial, int nb, double *out) {
  __shared__ double red[INT_WAVES];
  const double dnan = __builtin_nan("");
  double mn = dnan, mx = dnan, bad = 0;
  for (int i = threadIdx.x; i < nb; i += INT_THREADS) {
    mn = fmin(mn, partial[3 * i]);
    mx = fmax(mx, partial[3 * i + 1]);
    bad = fmax(bad, partial[3 * i + 2]);
  }
  mn = int_block_reduce(mn, red, OpMin());
  mx = int_block_reduce(mx, red, OpMax());
  bad = int_block_reduce(bad, red, OpMax());
  if (threadIdx.x == 0) {
    out[0] = bad != 0 ? dnan : mn;  // data.min() / data.max() propagate NaN
    out[1] = bad != 0 ? dnan : mx;
  }
}

template <typename T>
hipError_t launch_int_t(const IntLaunch &a, int path, size_t lds_bytes, hipStream_t s) {
  if (path == 0) {
    hipError_t e = hipFuncSetAttribute((const void *)intensity_kernel<T, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)INT_LDS_CAP);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((intensity_kernel<T, true>), dim3((unsigned)a.n), dim3(INT_THREADS), lds_bytes, s, a);
  } else {
    hipLaunchKernelGGL((intensity_kernel<T, false>), dim3((unsigned)a.n), dim3(INT_THREADS), 0, s, a);
  }
  return hipGetLastError();
}

template <typename T>
hipError_t launch_range_t(const void *src, int64_t count, double *partial, double *out, hipStream_t s) {
  const int64_t want = (count + INT_THREADS * 16 - 1) / (INT_THREADS * 16);
  const int nb = (int)(want < INT_RANGE_BLOCKS ? want : INT_RANGE_BLOCKS);
  hipLaunchKernelGGL(int_range_partial_kernel<T>, dim3((unsigned)nb), dim3(INT_THREADS), 0, s, (const T *)src, count,
                     partial);
  hipLaunchKernelGGL(int_range_final_kernel, dim3(1), dim3(INT_THREADS), 0, s, partial, nb, out);
  return hipGetLastError();
}

// kpdi_change_dtype: ndarray.astype, value by value (integers widen exactly to float64 first, so an integer-to-integer
// cast keeps the low bits as NumPy does)
template <typename T, typename TO>
__global__ __launch_bounds__(INT_THREADS) void change_dtype_kernel(const T *__restrict__ src, TO *__restrict__ dst,
                                                                   int64_t count) {
  using V = typename std::conditional<std::is_floating_point<T>::value, T, double>::type;
  for (int64_t i = (int64_t)blockIdx.x * INT_THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * INT_THREADS)
    dst[i] = astype_cast<TO>((V)src[i]);
}

template <typename T>
hipError_t launch_change_dtype_t(const void *src, void *dst, int dtype_out, int64_t count, hipStream_t s) {
  const int64_t want = (count + INT_THREADS * 8 - 1) / (INT_THREADS * 8);
  const unsigned nb = (unsigned)(want < 65536 ? want : 65536);
  return with_pattern_type(dtype_out, [&](auto o) {
    using TO = decltype(o);
    hipLaunchKernelGGL((change_dtype_kernel<T, TO>), dim3(nb), dim3(INT_THREADS), 0, s, (const T *)src, (TO *)dst, count);
    return hipGetLastError();
  });
}

}  // namespace

hipError_t launch_intensity(const IntLaunch &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const IntPlan plan = int_plan(a.dtype, a.sy, a.sx, a.n);
  if (plan.path < 0 || pattern_dtype_bytes(a.dtype_out) == 0 || !a.src || !a.dst) return hipErrorInvalidValue;
  if (a.dst == a.src && a.dtype_out != a.dtype) return hipErrorInvalidValue;  // only the same dtype works in place
  int path = plan.path;
  if (const char *e = getenv("KPDI_INTENSITY_PATH")) path = atoi(e) == 1 ? 1 : path;  // tests: path 1 for any shape
  return with_pattern_type(a.dtype, [&](auto t) { return launch_int_t<decltype(t)>(a, path, plan.lds_bytes, s); });
}

hipError_t launch_intensity_range(const void *src, int dtype, int64_t count, double *partial, double *out,
                                  hipStream_t s) {
  if (count <= 0 || !src || !partial || !out) return hipErrorInvalidValue;
  return with_pattern_type(dtype, [&](auto t) { return launch_range_t<decltype(t)>(src, count, partial, out, s); });
}

hipError_t launch_change_dtype(const void *src, int dtype, void *dst, int dtype_out, int64_t count, hipStream_t s) {
  if (count <= 0 || !src || !dst || src == dst) return hipErrorInvalidValue;
  return with_pattern_type(dtype, [&](auto t) { return launch_change_dtype_t<decltype(t)>(src, dst, dtype_out, count, s); });
}

}  // namespace kpdi
