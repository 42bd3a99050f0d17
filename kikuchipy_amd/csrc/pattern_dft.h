// pattern_dft.h - device helpers of the spectral pre-processing kernels (iq.hip, fftfilter.hip): the half-spectrum DFT of a
// real pattern and the workgroup reduction of per-pattern statistics.
//
// Half-spectrum DFT: p is real, so F(-k, -l) = conj F(k, l) and only the columns l = 0 ... sx/2 (half_cols) are
// transformed: a row DFT of length sx for those columns, then a column DFT of length sy over all k.  Twiddles come from
// a host table of f32 cos / sin of 2 pi j / N (computed in f64), indexed by the exact integer (k n) mod N; the sums run
// in f32 with explicit fmaf (this library builds with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "pattern_plan.h"

namespace kpdi {

// row DFT of one detector row at column frequency l: sum_x (row(x) - mean) e^{-2 pi i l x / sx}
template <typename Row>
__device__ __forceinline__ float2 row_dft(Row row, int sx, int l, float mean, const float2 *tw) {
  float re = 0.f, im = 0.f;
  int j = 0;
#pragma unroll 4
  for (int x = 0; x < sx; ++x) {
    const float v = row(x) - mean;
    const float2 t = tw[j];
    re = fmaf(v, t.x, re);
    im = fmaf(-v, t.y, im);
    j += l;
    j = j >= sx ? j - sx : j;
  }
  return make_float2(re, im);
}

// column DFT of the column `col` (stride h) at frequency k: sum_y col(y) e^{-+2 pi i k y / sy} (INV: +)
template <bool INV>
__device__ __forceinline__ float2 col_dft(const float2 *col, int h, int sy, int k, const float2 *tw) {
  float re = 0.f, im = 0.f;
  int j = 0;
#pragma unroll 4
  for (int y = 0; y < sy; ++y) {
    const float2 x = col[(size_t)y * h];
    const float2 t = tw[j];
    const float sn = INV ? t.y : -t.y;
    re = fmaf(x.x, t.x, fmaf(-x.y, sn, re));
    im = fmaf(x.y, t.x, fmaf(x.x, sn, im));
    j += k;
    j = j >= sy ? j - sy : j;
  }
  return make_float2(re, im);
}

// half spectrum -> real: sum_l Re(Y(l) e^{2 pi i l x / sx}) over the stored columns (the counts are folded into Y)
__device__ __forceinline__ float row_idft(const float2 *Y, int h, int sx, int x, const float2 *tw) {
  float v = 0.f;
  int j = 0;
#pragma unroll 4
  for (int l = 0; l < h; ++l) {
    const float2 y = Y[l], t = tw[j];
    v = fmaf(y.x, t.x, fmaf(-y.y, t.y, v));
    j += x;
    j = j >= sx ? j - sx : j;
  }
  return v;
}

// how often column l counts in the full spectrum: 1 for l = 0 and (even sx) l = sx/2, whose mirrors are themselves, else 2
template <typename V>
__device__ __forceinline__ V column_count(int l, int sx) { return (l == 0 || 2 * l == sx) ? V(1) : V(2); }

// the combining operations of block_reduce, with their identities
struct RedSum {
  template <typename T> static __device__ __forceinline__ T id() { return T(0); }
  template <typename T> static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
struct RedMin {
  template <typename T> static __device__ __forceinline__ T id() { return __builtin_inff(); }
  template <typename T> static __device__ __forceinline__ T op(T a, T b) { return fminf(a, b); }
};
struct RedMax {
  template <typename T> static __device__ __forceinline__ T id() { return -__builtin_inff(); }
  template <typename T> static __device__ __forceinline__ T op(T a, T b) { return fmaxf(a, b); }
};
struct RedOr {
  template <typename T> static __device__ __forceinline__ T id() { return T(0); }
  template <typename T> static __device__ __forceinline__ T op(T a, T b) { return a | b; }
};

// reduces each value v[i] with Ops[i] over a workgroup of WAVES waves; every thread gets the results.  Within a wave an
// xor butterfly 32 ... 1; then, from the identity, the waves' results in wave order.  `red`: sizeof...(v) doubles per
// wave, which may still be read from a previous use (hence the first barrier).
template <int WAVES, typename... Ops, typename... T>
__device__ __forceinline__ void block_reduce(double *red, T &...v) {
  static_assert(sizeof...(Ops) == sizeof...(T), "one operation per value");
  constexpr int K = sizeof...(T);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) ((v = Ops::op(v, __shfl_xor(v, o, 64))), ...);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    int j = K * w;
    ((red[j++] = v), ...);
  }
  __syncthreads();
  ((v = Ops::template id<T>()), ...);
  for (int i = 0; i < WAVES; ++i) {
    int j = K * i;
    ((v = Ops::op(v, (T)red[j++])), ...);
  }
}

}  // namespace kpdi
