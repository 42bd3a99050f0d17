// decomp.hip - the device side of the PCA decomposition of the resident patterns (EBSD.decomposition,
// EBSD.get_decomposition_model; signals/ebsd.py:2665-2723, signals/util/_dask.py:283-332): the float64 Gram matrix of the
// centred pattern matrix, the products of the centred patterns with a basis, and the model sum_j l[m, j] f[k, j] + mean
// written back as the resident patterns.  The eigen-solve between them runs on the host.
//
// X is the M x K matrix of the patterns (K = sy sx, row-major pixels), every value widened exactly to float64.
// Centring subtracts a mean when a tile is staged, xc = double(x) - mean rounded once; the centred matrix never exists
// in memory.  The means come from two small pre-kernels, float64 sums in a fixed order, no atomics, divided once:
//   "signal" (one mean per pattern): thread t of 256 adds pixels t, t + 256, ... in turn; then block_reduce's tree
//       (xor butterfly 32 ... 1 within a wave, then the four waves in order); / K.
//   "navigation" (the mean pattern): per pixel, the rows of each block of DEC_MEAN_ROWS patterns in turn, then the
//       blocks' partial sums in turn; / M.
//
// All three products are ONE tile kernel (dec_tile_kernel) on v_mfma_f64_16x16x4_f64.  A workgroup of 4 waves owns a 64 x
// 64 output tile; per stage both operands' DEC_KB x 64 slices are converted to float64 (and centred) on their way into
// LDS as S[r][o] (reduction index r, output index o); a wave owns 32 x 32 outputs = 2 x 2 MFMA blocks whose accumulators
// (4 x 4 doubles per lane, 32 VGPRs) stay in registers over the whole reduction.  Lane l feeds A[i = l & 15][k = l >> 4]
// and B[k = l >> 4][j = l & 15]; result register g of lane l is D[row = (l >> 4) + 4 g][col = l & 15] - the f64 map, not
// the f32 one.  Each output is one chain of MFMAs over the stages in order: no split reduction, no atomics, nothing that
// depends on the launch.  Rows, columns and reduction steps beyond the matrices are zeros in LDS (a centred zero would be
// -mean) and their outputs are not stored.  Tile and limit arithmetic: decomp_plan.h.
#include "../../include/kpdi.h"
#include "decomp_plan.h"
#include "kernels.h"
#include "pattern_dft.h"
#include "prep_device.h"

#include <type_traits>

namespace kpdi {

namespace {

typedef double dec_d4 __attribute__((ext_vector_type(4)));

// operand whose reduction index is the ROW of a row-major [nr][no] matrix (the patterns for X^T ..., a basis)
template <typename T>
struct DecCol {
  const T *src;
  int64_t nr, no;
  const double *mean_row, *mean_col;  // either may be set: subtracted from every value of its row / column
  __device__ __forceinline__ void stage(double *S, int64_t o0, int64_t r0) const {
    const int i = threadIdx.x & 63;
    const int64_t go = o0 + i;
#pragma unroll
    for (int q = 0; q < DEC_KB / 4; ++q) {
      const int r = (threadIdx.x >> 6) + 4 * q;
      const int64_t gr = r0 + r;
      double v = 0.0;
      if (gr < nr && go < no) {
        v = (double)src[gr * no + go];
        if (mean_row) v -= mean_row[gr];
        if (mean_col) v -= mean_col[go];
      }
      S[r * DEC_LD + i] = v;
    }
  }
};

// operand whose reduction index is the COLUMN of a row-major [no][nr] matrix (the patterns for X ..., loadings, factors)
template <typename T>
struct DecRow {
  const T *src;
  int64_t no, nr;
  const double *mean_row, *mean_col;
  __device__ __forceinline__ void stage(double *S, int64_t o0, int64_t r0) const {
    const int r = threadIdx.x & (DEC_KB - 1);
    const int64_t gr = r0 + r;
#pragma unroll
    for (int q = 0; q < DEC_TILE * DEC_KB / DEC_THREADS; ++q) {
      const int i = (threadIdx.x >> 4) + (DEC_THREADS / DEC_KB) * q;
      const int64_t go = o0 + i;
      double v = 0.0;
      if (gr < nr && go < no) {
        v = (double)src[go * nr + gr];
        if (mean_row) v -= mean_row[go];
        if (mean_col) v -= mean_col[gr];
      }
      S[r * DEC_LD + i] = v;
    }
  }
};

// epilogues: what becomes of output (i, j)
struct DecStore {  // out[ni][nj]
  double *out;
  int64_t ni, nj;
  static constexpr bool symmetric = false;
  __device__ __forceinline__ void operator()(int64_t i, int64_t j, double v) const {
    if (i < ni && j < nj) out[i * nj + j] = v;
  }
};
struct DecStoreSym {  // out[n][n]: the upper triangle is computed, both triangles are written
  double *out;
  int64_t n;
  static constexpr bool symmetric = true;
  __device__ __forceinline__ void operator()(int64_t i, int64_t j, double v) const {
    if (i < n && j < n && j >= i) {
      out[i * n + j] = v;
      out[j * n + i] = v;
    }
  }
};
template <typename TO>
struct DecStoreModel {  // out[ni][nj] = TO(v + mean), rounded once
  TO *out;
  int64_t ni, nj;
  const double *mean_row, *mean_col;
  static constexpr bool symmetric = false;
  __device__ __forceinline__ void operator()(int64_t i, int64_t j, double v) const {
    if (i < ni && j < nj) {
      if (mean_row) v += mean_row[i];
      if (mean_col) v += mean_col[j];
      out[i * nj + j] = astype_cast<TO>(v);
    }
  }
};

// out(i, j) = sum_r A(r, i) B(r, j) for the 64 x 64 tile blockIdx.x of a tiles_j-wide tile grid
template <typename LA, typename LB, typename EP>
__global__ __launch_bounds__(DEC_THREADS) void dec_tile_kernel(LA la, LB lb, EP ep, int64_t nreduce, int tiles_j) {
  __shared__ double As[DEC_KB * DEC_LD];
  __shared__ double Bs[DEC_KB * DEC_LD];
  const int ti = (int)(blockIdx.x / (unsigned)tiles_j), tj = (int)(blockIdx.x % (unsigned)tiles_j);
  if (EP::symmetric && tj < ti) return;  // the mirror tile writes these
  const int64_t i0 = (int64_t)ti * DEC_TILE, j0 = (int64_t)tj * DEC_TILE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wi = (w >> 1) * 32, wj = (w & 1) * 32;
  const int lk = lane >> 4, lo = lane & 15;
  dec_d4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = dec_d4{0.0, 0.0, 0.0, 0.0};
  for (int64_t r0 = 0; r0 < nreduce; r0 += DEC_KB) {
    la.stage(As, i0, r0);
    lb.stage(Bs, j0, r0);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < DEC_KB / 4; ++kk) {
      const double *ar = As + (kk * 4 + lk) * DEC_LD + wi + lo;
      const double *br = Bs + (kk * 4 + lk) * DEC_LD + wj + lo;
      const double a0 = ar[0], a1 = ar[16], b0 = br[0], b1 = br[16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();  // the next stage overwrites the slices
  }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int g = 0; g < 4; ++g) ep(i0 + wi + 16 * x + lk + 4 * g, j0 + wj + 16 * y + lo, acc[x][y][g]);
}

template <typename LA, typename LB, typename EP>
hipError_t launch_tiles(const LA &la, const LB &lb, const EP &ep, int64_t ni, int64_t nj, int64_t nreduce, hipStream_t s) {
  const int64_t tiles_i = dec_tiles(ni), tiles_j = dec_tiles(nj);
  if (ni < 1 || nj < 1 || nreduce < 1 || tiles_i * tiles_j >= (int64_t)INT32_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL((dec_tile_kernel<LA, LB, EP>), dim3((unsigned)(tiles_i * tiles_j)), dim3(DEC_THREADS), 0, s, la, lb, ep,
                     nreduce, (int)tiles_j);
  return hipGetLastError();
}

// ---- means ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(DEC_THREADS) void dec_mean_signal_kernel(const T *__restrict__ src, int64_t k, double *mean) {
  __shared__ double red[DEC_THREADS / 64];
  const T *p = src + (int64_t)blockIdx.x * k;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < k; i += DEC_THREADS) s += (double)p[i];
  block_reduce<DEC_THREADS / 64, RedSum>(red, s);
  if (threadIdx.x == 0) mean[blockIdx.x] = s / (double)k;
}

// partial[chunk][pixel]: the rows of block `chunk` of DEC_MEAN_ROWS patterns, in turn
template <typename T>
__global__ __launch_bounds__(DEC_THREADS) void dec_mean_nav_partial_kernel(const T *__restrict__ src, int64_t m, int64_t k,
                                                                            int kblocks, double *partial) {
  const int64_t chunk = blockIdx.x / (unsigned)kblocks;
  const int64_t pix = (int64_t)(blockIdx.x % (unsigned)kblocks) * DEC_THREADS + threadIdx.x;
  if (pix >= k) return;
  const int64_t m0 = chunk * DEC_MEAN_ROWS, m1 = m0 + DEC_MEAN_ROWS < m ? m0 + DEC_MEAN_ROWS : m;
  double s = 0.0;
  for (int64_t r = m0; r < m1; ++r) s += (double)src[r * k + pix];
  partial[chunk * k + pix] = s;
}

__global__ __launch_bounds__(DEC_THREADS) void dec_mean_nav_final_kernel(const double *__restrict__ partial, int64_t chunks,
                                                                          int64_t m, int64_t k, double *mean) {
  const int64_t pix = (int64_t)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (pix >= k) return;
  double s = 0.0;
  for (int64_t c = 0; c < chunks; ++c) s += partial[c * k + pix];
  mean[pix] = s / (double)m;
}

template <typename T>
hipError_t launch_means_t(const DecLaunch &a, hipStream_t s) {
  const T *src = (const T *)a.patterns;
  if (a.centre == DEC_CENTRE_SIGNAL) {
    hipLaunchKernelGGL(dec_mean_signal_kernel<T>, dim3((unsigned)a.m), dim3(DEC_THREADS), 0, s, src, a.k, a.mean);
  } else {
    const int64_t chunks = dec_mean_chunks(a.m), kblocks = (a.k + DEC_THREADS - 1) / DEC_THREADS;
    if (chunks * kblocks >= (int64_t)INT32_MAX || !a.mean_partial) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_mean_nav_partial_kernel<T>, dim3((unsigned)(chunks * kblocks)), dim3(DEC_THREADS), 0, s, src, a.m,
                       a.k, (int)kblocks, a.mean_partial);
    hipLaunchKernelGGL(dec_mean_nav_final_kernel, dim3((unsigned)kblocks), dim3(DEC_THREADS), 0, s, a.mean_partial, chunks, a.m,
                       a.k, a.mean);
  }
  return hipGetLastError();
}

template <typename T>
hipError_t launch_gram_t(const DecLaunch &a, int transposed, double *gram, hipStream_t s) {
  const double *mr = a.centre == DEC_CENTRE_SIGNAL ? a.mean : nullptr, *mc = a.centre == DEC_CENTRE_NAVIGATION ? a.mean : nullptr;
  const T *src = (const T *)a.patterns;
  if (transposed) {  // X X^T: the reduction runs along the pixels
    const DecRow<T> x{src, a.m, a.k, mr, mc};
    return launch_tiles(x, x, DecStoreSym{gram, a.m}, a.m, a.m, a.k, s);
  }
  const DecCol<T> x{src, a.m, a.k, mr, mc};  // X^T X: down the patterns
  return launch_tiles(x, x, DecStoreSym{gram, a.k}, a.k, a.k, a.m, s);
}

template <typename T>
hipError_t launch_apply_t(const DecLaunch &a, int transposed_op, const double *basis, int c, double *out, hipStream_t s) {
  const double *mr = a.centre == DEC_CENTRE_SIGNAL ? a.mean : nullptr, *mc = a.centre == DEC_CENTRE_NAVIGATION ? a.mean : nullptr;
  const T *src = (const T *)a.patterns;
  if (transposed_op) {  // Xc^T basis: [K][c] from a basis of [M][c]
    const DecCol<T> x{src, a.m, a.k, mr, mc};
    const DecCol<double> b{basis, a.m, c, nullptr, nullptr};
    return launch_tiles(x, b, DecStore{out, a.k, c}, a.k, c, a.m, s);
  }
  const DecRow<T> x{src, a.m, a.k, mr, mc};  // Xc basis: [M][c] from a basis of [K][c]
  const DecCol<double> b{basis, a.k, c, nullptr, nullptr};
  return launch_tiles(x, b, DecStore{out, a.m, c}, a.m, c, a.k, s);
}

template <typename D>
hipError_t launch_model_t(const DecModelLaunch &a, hipStream_t s) {
  const DecRow<D> l{(const D *)a.loadings, a.m, a.c, nullptr, nullptr}, f{(const D *)a.factors, a.k, a.c, nullptr, nullptr};
  const DecStoreModel<D> ep{(D *)a.dst, a.m, a.k, a.mean_kind == DEC_CENTRE_SIGNAL ? a.mean : nullptr,
                            a.mean_kind == DEC_CENTRE_NAVIGATION ? a.mean : nullptr};
  return launch_tiles(l, f, ep, a.m, a.k, a.c, s);
}

bool dec_launch_ok(const DecLaunch &a) {
  return a.patterns && a.m >= 1 && a.k >= 1 && a.centre >= DEC_CENTRE_NONE && a.centre <= DEC_CENTRE_SIGNAL &&
         (a.centre == DEC_CENTRE_NONE || a.mean);
}

}  // namespace

hipError_t launch_decomposition_means(const DecLaunch &a, hipStream_t s) {
  if (!dec_launch_ok(a) || a.centre == DEC_CENTRE_NONE) return hipErrorInvalidValue;
  return with_pattern_type(a.dtype, [&](auto t) { return launch_means_t<decltype(t)>(a, s); });
}

hipError_t launch_decomposition_gram(const DecLaunch &a, int transposed, double *gram, hipStream_t s) {
  if (!dec_launch_ok(a) || !gram) return hipErrorInvalidValue;
  return with_pattern_type(a.dtype, [&](auto t) { return launch_gram_t<decltype(t)>(a, transposed, gram, s); });
}

hipError_t launch_decomposition_apply(const DecLaunch &a, int transposed_op, const double *basis, int c, double *out,
                                      hipStream_t s) {
  if (!dec_launch_ok(a) || !basis || !out || c < 1) return hipErrorInvalidValue;
  return with_pattern_type(a.dtype, [&](auto t) { return launch_apply_t<decltype(t)>(a, transposed_op, basis, c, out, s); });
}

hipError_t launch_decomposition_model(const DecModelLaunch &a, hipStream_t s) {
  if (!a.loadings || !a.factors || !a.dst || a.m < 1 || a.k < 1 || a.c < 1) return hipErrorInvalidValue;
  if (a.mean && a.mean_kind != DEC_CENTRE_NAVIGATION && a.mean_kind != DEC_CENTRE_SIGNAL) return hipErrorInvalidValue;
  if (a.dtype_out == KPDI_F32) return launch_model_t<float>(a, s);
  if (a.dtype_out == KPDI_F64) return launch_model_t<double>(a, s);
  return hipErrorInvalidValue;
}

}  // namespace kpdi
