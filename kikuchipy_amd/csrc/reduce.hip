// reduce.hip - sum, mean, max, min, std and var of the resident patterns (ny, nx, sy, sx) over any set of their axes
// (EBSD.sum / mean / max / min / std / var): a read of every byte, bound by HBM.  The form in[A][R1][M][R2][B] ->
// out[A][M][B] of an axis set, the two regimes, the slices and the launch geometry: reduce_plan.h.
//   red_cols_kernel (B > 1): a lane owns 16 bytes of a row of B - one load of any alignment, as select.hip's - and an
//     accumulator per element; it walks the rows r = lo ... hi of its slice, four loads in flight.
//   red_runs_kernel (B == 1): `group` lanes share an output; vector j of a run's part in the slice goes to lane j % group,
//     which adds its elements in order; the lanes are combined by the xor butterfly group/2 ... 1.
//   red_combine_kernel: one lane per output combines its partials in slice order and finishes the op; past
//     RED_COMBINE_SERIAL slices, RED_COMBINE_LANES lanes share them (with one lane walking the 512 slices of a 256 x 256
//     map's mean pattern, the uint8 reduction measured 0.172 ms; with 16, 0.057 ms).
// A pass is a partial kernel and a combine kernel; std / var of float patterns take two (the float64 mean, then the
// squared deviations from it).  Every value is read by exactly one (slice, lane), nothing is written but the workspace.
// Arithmetic: integer patterns add x (and x^2 for std / var) exactly in uint64 / int64, and var = (n sum x^2 - (sum x)^2)
// / n^2 is taken from the exact 128-bit numerator; float patterns are widened to float64 (exact) and added, subtracted
// and multiplied there - the build has -ffp-contract=off - and the result is rounded once to the output.  max / min
// stay in the dtype; a NaN, once met, stays (x != x is kept by every later comparison).  No atomics; LDS only where the
// lanes of the combine kernel meet.
#include <limits>
#include <type_traits>

#include "../../include/kpdi.h"
#include "kernels.h"
#include "reduce_plan.h"

namespace kpdi {

namespace {

typedef unsigned long long red_word;  // a partial: the bits of a uint64 / int64 / float64

struct RedArgs {
  const void *src;
  red_word *partial;   // [plane][slice][output]
  const double *mean;  // [output], RED_PHASE_DEV2
  RedShape sh;
  int64_t n_out, n_red, slice, vb, items;
  int n_slices, group;
};

template <typename T, int PH>
struct RedAcc {
  static constexpr bool F = std::is_floating_point<T>::value;
  static constexpr bool EXT = PH == RED_PHASE_MAX || PH == RED_PHASE_MIN;
  using Sum = std::conditional_t<F, double, std::conditional_t<std::is_signed<T>::value, long long, unsigned long long>>;
  using W = std::conditional_t<EXT, T, Sum>;
  W a;
  unsigned long long q;  // RED_PHASE_SUMSQ: sum x^2

  __device__ __forceinline__ void init() {
    q = 0;
    if constexpr (PH == RED_PHASE_MAX) a = F ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::lowest();
    else if constexpr (PH == RED_PHASE_MIN) a = F ? std::numeric_limits<T>::infinity() : std::numeric_limits<T>::max();
    else a = 0;
  }
  // the larger (smaller) of the two, a NaN before anything
  static __device__ __forceinline__ T pick(T x, T m) {
    if constexpr (PH == RED_PHASE_MAX) return (x > m || x != x) ? x : m;
    else return (x < m || x != x) ? x : m;
  }
  __device__ __forceinline__ void add(T x, double mu) {
    if constexpr (EXT) {
      a = pick(x, a);
    } else if constexpr (PH == RED_PHASE_DEV2) {
      const double d = (double)x - mu;
      a += d * d;
    } else {
      a += (Sum)x;
      if constexpr (PH == RED_PHASE_SUMSQ) {
        const long long v = (long long)x;
        q += (unsigned long long)(v * v);
      }
    }
  }
  __device__ __forceinline__ void merge(const RedAcc &o) {
    if constexpr (EXT) {
      a = pick(o.a, a);
    } else {
      a += o.a;
      q += o.q;
    }
  }
  __device__ __forceinline__ red_word bits() const {
    if constexpr (F) return (red_word)__double_as_longlong((double)a);
    else return (red_word)(long long)a;
  }
  __device__ __forceinline__ void from_bits(red_word w) {
    if constexpr (F) a = (W)__longlong_as_double((long long)w);
    else a = (W)(long long)w;
  }
};

// 16 bytes from an address of any alignment, as naturally aligned loads (select.hip's sel_load16)
__device__ __forceinline__ uint4 red_load16(const unsigned char *p) {
  const unsigned al = (unsigned)(uintptr_t)p & 15u;
  if (al == 0) return *reinterpret_cast<const uint4 *>(p);
  if ((al & 7u) == 0) {
    const uint2 lo = reinterpret_cast<const uint2 *>(p)[0], hi = reinterpret_cast<const uint2 *>(p)[1];
    return make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
  unsigned w[4];
  if ((al & 3u) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const unsigned *>(p)[k];
  } else if ((al & 1u) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned short *h = reinterpret_cast<const unsigned short *>(p) + 2 * k;
      w[k] = (unsigned)h[0] | ((unsigned)h[1] << 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      w[k] = (unsigned)p[4 * k] | ((unsigned)p[4 * k + 1] << 8) | ((unsigned)p[4 * k + 2] << 16) | ((unsigned)p[4 * k + 3] << 24);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <typename T>
struct RedVec {
  static constexpr int V = 16 / (int)sizeof(T);
  T x[V];
  __device__ __forceinline__ void load(const T *p) {
    const uint4 w = red_load16(reinterpret_cast<const unsigned char *>(p));
    __builtin_memcpy(x, &w, 16);
  }
};

template <typename T, int PH>
__global__ __launch_bounds__(RED_THREADS) void red_cols_kernel(RedArgs a) {
  constexpr int V = RedVec<T>::V;
  const int64_t item = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x;
  if (item >= a.items) return;
  int64_t am, b0;
  int count;
  red_cols_item(item, a.vb, V, a.sh.B, &am, &b0, &count);
  const int64_t aa = am / a.sh.M, m = am - aa * a.sh.M, o = am * a.sh.B + b0;
  int64_t lo, hi;
  red_slice_bounds(a.n_red, a.slice, (int)blockIdx.y, &lo, &hi);
  int64_t r1 = lo / a.sh.R2, r2 = lo - r1 * a.sh.R2;
  const T *p = (const T *)a.src + red_element(a.sh, aa, r1, m, r2, b0);
  const int64_t next_run = (a.sh.M - 1) * a.sh.R2 * a.sh.B;  // from the end of a run of R2 rows to the next r1's
  RedAcc<T, PH> acc[V];
  double mu[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    acc[j].init();
    mu[j] = PH == RED_PHASE_DEV2 && j < count ? a.mean[o + j] : 0.0;
  }
  for (int64_t r = lo; r < hi;) {
    int64_t n = a.sh.R2 - r2 < hi - r ? a.sh.R2 - r2 : hi - r;  // rows of this run: B apart
    r += n;
    r2 += n;
    if (count == V) {
      for (; n >= 4; n -= 4, p += 4 * a.sh.B) {
        RedVec<T> v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k].load(p + k * a.sh.B);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
          for (int j = 0; j < V; ++j) acc[j].add(v[k].x[j], mu[j]);
      }
      for (; n > 0; --n, p += a.sh.B) {
        RedVec<T> v;
        v.load(p);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j].add(v.x[j], mu[j]);
      }
    } else {  // the cut vector at the end of a row of B
      for (; n > 0; --n, p += a.sh.B) {
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (j < count) acc[j].add(p[j], mu[j]);
      }
    }
    if (r2 == a.sh.R2) {
      r2 = 0;
      p += next_run;  // (only dereferenced while r < hi)
    }
  }
  red_word *dst = a.partial + (int64_t)blockIdx.y * a.n_out + o;
#pragma unroll
  for (int j = 0; j < V; ++j)
    if (j < count) {
      dst[j] = acc[j].bits();
      if constexpr (PH == RED_PHASE_SUMSQ) dst[(int64_t)a.n_slices * a.n_out + j] = acc[j].q;
    }
}

template <typename T, int PH>
__global__ __launch_bounds__(RED_THREADS) void red_runs_kernel(RedArgs a) {
  constexpr int V = RedVec<T>::V;
  const int64_t t = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x;
  const int64_t o = t / a.group;
  const int g = (int)(t - o * a.group);
  const bool valid = o < a.n_out;  // (a lane without an output still takes part in the butterfly)
  RedAcc<T, PH> acc;
  acc.init();
  if (valid) {
    const int64_t aa = o / a.sh.M, m = o - aa * a.sh.M;
    const double mu = PH == RED_PHASE_DEV2 ? a.mean[o] : 0.0;
    int64_t lo, hi;
    red_slice_bounds(a.n_red, a.slice, (int)blockIdx.y, &lo, &hi);
    for (int64_t r1 = lo / a.sh.R2; r1 * a.sh.R2 < hi; ++r1) {
      const int64_t e0 = lo > r1 * a.sh.R2 ? lo - r1 * a.sh.R2 : 0;                    // the run's part in the slice:
      const int64_t e1 = hi < (r1 + 1) * a.sh.R2 ? hi - r1 * a.sh.R2 : a.sh.R2;        // its values [e0, e1)
      const T *run = (const T *)a.src + red_element(a.sh, aa, r1, m, 0, 0);
      const int64_t nvec = (e1 - e0 + V - 1) / V;
      for (int64_t j = g; j < nvec; j += a.group) {  // (red_runs_lane(j, group) == g)
        const int64_t e = e0 + j * V;
        if (e + V <= e1) {
          RedVec<T> v;
          v.load(run + e);
#pragma unroll
          for (int k = 0; k < V; ++k) acc.add(v.x[k], mu);
        } else {
          for (int64_t k = e; k < e1; ++k) acc.add(run[k], mu);
        }
      }
    }
  }
  for (int off = a.group >> 1; off >= 1; off >>= 1) {
    RedAcc<T, PH> other;
    other.from_bits(__shfl_xor(acc.bits(), off, 64));
    other.q = __shfl_xor(acc.q, off, 64);
    acc.merge(other);
  }
  if (valid && g == 0) {
    red_word *dst = a.partial + (int64_t)blockIdx.y * a.n_out + o;
    dst[0] = acc.bits();
    if constexpr (PH == RED_PHASE_SUMSQ) dst[(int64_t)a.n_slices * a.n_out] = acc.q;
  }
}

// the partials of an output, then the op; `mean_out`: the float64 mean is all this pass is for.  `lanes` (1 or
// RED_COMBINE_LANES) lanes share an output: lane g combines the slices g, g + lanes, ... in that order, lane 0 then the
// lanes in lane order (through LDS).  A workgroup takes RED_THREADS / lanes neighbouring outputs, so the lanes of one g
// read neighbouring words.
template <typename T, int PH>
__global__ __launch_bounds__(RED_THREADS) void red_combine_kernel(const red_word *__restrict__ partial, int64_t n_out,
                                                                  int n_slices, int lanes, int op, int64_t n_red,
                                                                  double *__restrict__ mean_out, void *__restrict__ out) {
  using Acc = RedAcc<T, PH>;
  __shared__ red_word shared[2][RED_THREADS];
  const int per_block = RED_THREADS / lanes, g = threadIdx.x / per_block;
  const int64_t o = (int64_t)blockIdx.x * per_block + (threadIdx.x - g * per_block);
  const bool valid = o < n_out;  // (n_slices >= lanes: every lane has a first slice)
  Acc acc;
  acc.init();
  if (valid) {
    acc.from_bits(partial[(int64_t)g * n_out + o]);
    acc.q = PH == RED_PHASE_SUMSQ ? partial[((int64_t)n_slices + g) * n_out + o] : 0;
    for (int s = g + lanes; s < n_slices; s += lanes) {
      Acc other;
      other.from_bits(partial[(int64_t)s * n_out + o]);
      other.q = PH == RED_PHASE_SUMSQ ? partial[((int64_t)n_slices + s) * n_out + o] : 0;
      acc.merge(other);
    }
  }
  if (lanes > 1) {  // (uniform)
    shared[0][threadIdx.x] = acc.bits();
    shared[1][threadIdx.x] = acc.q;
    __syncthreads();
    if (g == 0)
      for (int k = 1; k < lanes; ++k) {
        Acc other;
        other.from_bits(shared[0][k * per_block + threadIdx.x]);
        other.q = shared[1][k * per_block + threadIdx.x];
        acc.merge(other);
      }
  }
  if (!valid || g != 0) return;
  const double n = (double)n_red;
  if constexpr (Acc::EXT) {
    ((T *)out)[o] = acc.a;
  } else if constexpr (Acc::F) {
    double v = acc.a;
    if (PH == RED_PHASE_DEV2 || op != KPDI_REDUCE_SUM) v = v / n;
    if (mean_out) {
      mean_out[o] = v;
      return;
    }
    if (op == KPDI_REDUCE_STD) v = sqrt(v);
    ((T *)out)[o] = (T)v;
  } else if constexpr (PH == RED_PHASE_SUM) {
    if (op == KPDI_REDUCE_SUM) ((typename Acc::Sum *)out)[o] = acc.a;
    else ((double *)out)[o] = (double)acc.a / n;
  } else {  // RED_PHASE_SUMSQ: n sum x^2 - (sum x)^2 >= 0, exactly; four roundings from there to the variance
    const unsigned long long s1 = acc.a < 0 ? 0ull - (unsigned long long)acc.a : (unsigned long long)acc.a;
    const unsigned __int128 d = (unsigned __int128)(unsigned long long)n_red * acc.q - (unsigned __int128)s1 * s1;
    double v = (double)(unsigned long long)(d >> 64) * 18446744073709551616.0 + (double)(unsigned long long)d;
    v = v / n / n;
    if (op == KPDI_REDUCE_STD) v = sqrt(v);
    ((double *)out)[o] = v;
  }
}

template <typename T, int PH>
hipError_t launch_pass(const RedArgs &a, const RedPlan &p, int op, double *mean_out, void *out, hipStream_t s) {
  const dim3 grid(p.grid_x, p.grid_y), block(RED_THREADS);
  if (p.regime == RED_COLS) hipLaunchKernelGGL((red_cols_kernel<T, PH>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((red_runs_kernel<T, PH>), grid, block, 0, s, a);
  const int64_t per_block = RED_THREADS / p.combine_lanes;
  hipLaunchKernelGGL((red_combine_kernel<T, PH>), dim3((unsigned)((p.n_out + per_block - 1) / per_block)), block, 0, s,
                     a.partial, p.n_out, p.n_slices, p.combine_lanes, op, p.n_red, mean_out, out);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_reduce_t(const RedLaunch &l, const RedPlan &p, hipStream_t s) {
  char *ws = (char *)l.workspace;
  RedArgs a{};
  a.src = l.patterns;
  a.partial = (red_word *)ws;
  a.mean = (const double *)(ws + p.mean_off);
  a.sh = p.sh;
  a.n_out = p.n_out;
  a.n_red = p.n_red;
  a.slice = p.slice;
  a.vb = p.vb;
  a.items = p.items;
  a.n_slices = p.n_slices;
  a.group = p.group;
  void *out = ws + p.out_off;
  switch (l.op) {
    case KPDI_REDUCE_SUM:
    case KPDI_REDUCE_MEAN: return launch_pass<T, RED_PHASE_SUM>(a, p, l.op, nullptr, out, s);
    case KPDI_REDUCE_MAX: return launch_pass<T, RED_PHASE_MAX>(a, p, l.op, nullptr, out, s);
    case KPDI_REDUCE_MIN: return launch_pass<T, RED_PHASE_MIN>(a, p, l.op, nullptr, out, s);
    default: break;
  }
  if constexpr (std::is_floating_point<T>::value) {
    hipError_t e = launch_pass<T, RED_PHASE_SUM>(a, p, KPDI_REDUCE_MEAN, (double *)(ws + p.mean_off), nullptr, s);
    if (e != hipSuccess) return e;
    return launch_pass<T, RED_PHASE_DEV2>(a, p, l.op, nullptr, out, s);
  } else {
    return launch_pass<T, RED_PHASE_SUMSQ>(a, p, l.op, nullptr, out, s);
  }
}

}  // namespace

hipError_t launch_reduce(const RedLaunch &l, hipStream_t s) {
  const RedPlan p = reduce_plan(l.dtype, l.op, l.axis_mask, l.ny, l.nx, l.sy, l.sx);
  if (p.regime < 0 || !l.patterns || !l.workspace || l.workspace_bytes < p.workspace_bytes) return hipErrorInvalidValue;
  return with_pattern_type(l.dtype, [&](auto t) { return launch_reduce_t<decltype(t)>(l, p, s); });
}

}  // namespace kpdi
