// orientations.hip - disorientation angles, zone reduction and kernel average misorientation (KAM) maps of orientations
// under the proper operations of their point groups (kikuchipy_amd/orientations.py), in float64.
// What one pair, one orientation or one map point computes, and the launch arithmetic, are in orientations_plan.h, the
// same C++ a host test compiles.  The operation tables (at most 24 x 4 doubles per group) are kernel arguments.
//
//   pairs:  one thread per output of a broadcast call; the rows of the two inputs from strides (0 where broadcast).
//   outer:  N x M angles.  A workgroup of 4 waves owns a 32 x 32 tile; it stages the equivalents s1 g1 of its 32 rows and
//           s2 g2 of its 32 columns in LDS once (normalised on the way), a wave owns one 16 x 16 block.  The candidate
//           search is the K = 4 inner product: one v_mfma_f64_16x16x4_f64 per (s1, s2) gives the 256 dot products of the
//           block, each lane keeps the largest |.| of its four outputs and the candidate's index (the lowest among equal
//           maxima).  Lane l feeds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result register g of lane l
//           is D[row = (l >> 4) + 4 g][col = l & 15] (the float64 map of decomp.hip).  The winner is evaluated again from
//           LDS as the product (s2 g2)(s1 g1)^-1 and its angle 2 atan2(|v|, |w|) goes through an LDS tile so that a thread
//           stores four consecutive outputs of a row, a row of the tile leaving as one contiguous run.  64-bit output
//           indices, no atomics, every output written by exactly one thread.
//   reduce: one thread per orientation.   KAM: one thread per map point, the window's offsets in a small table.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "orientations_plan.h"

namespace kpdi {

namespace {

typedef double ori_d4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(ORI_THREADS) void orientation_pairs_kernel(const double *q1, const double *q2, OriShape shape,
                                                                        int64_t count, OriOps ops1, OriOps ops2, double scale,
                                                                        double *out) {
  const int64_t p = (int64_t)blockIdx.x * ORI_THREADS + threadIdx.x;
  if (p >= count) return;
  int64_t r1, r2;
  ori_pair_rows(p, shape, &r1, &r2);
  double g1[4], g2[4];
  ori_normalise(q1 + 4 * r1, g1);
  ori_normalise(q2 + 4 * r2, g2);
  out[p] = ori_pair_angle(g1, g2, ops1, ops2, nullptr) * scale;
}

__global__ __launch_bounds__(ORI_THREADS) void orientation_reduce_kernel(const double *q, int64_t n, OriOps ops, double *out,
                                                                         int32_t *index) {
  const int64_t p = (int64_t)blockIdx.x * ORI_THREADS + threadIdx.x;
  if (p >= n) return;
  double r[4];
  const int at = ori_reduce(q + 4 * p, ops, r);
  double2 *dst = reinterpret_cast<double2 *>(out + 4 * p);
  dst[0] = make_double2(r[0], r[1]);
  dst[1] = make_double2(r[2], r[3]);
  index[p] = at;
}

__global__ __launch_bounds__(ORI_THREADS) void orientation_kam_kernel(const double *rot, int ny, int nx, OriOps one, OriOps ops,
                                                                      const int32_t *offsets, int n_offsets,
                                                                      const uint8_t *in_data, double max_angle, double scale,
                                                                      double *out) {
  const int64_t p = (int64_t)blockIdx.x * ORI_THREADS + threadIdx.x;
  if (p >= (int64_t)ny * nx) return;
  out[p] = ori_kam_point(rot, ny, nx, (int)(p / nx), (int)(p % nx), one, ops, offsets, n_offsets, in_data, max_angle) * scale;
}

// the equivalents of `rows` rows from `first` on (of `total`), normalised, into S[op][row of the tile][4]; rows beyond the
// set are NaN (their outputs are never stored)
__device__ inline void stage_equivalents(const double *q, int64_t first, int64_t total, int rows, const OriOps &ops, double *S) {
  for (int t = threadIdx.x; t < ops.n * rows; t += ORI_THREADS) {
    const int s = t / rows, r = t - s * rows;
    const int64_t row = first + r;
    const double nan4[4] = {nan(""), nan(""), nan(""), nan("")};
    double g[4], e[4];
    if (row < total)
      ori_normalise(q + 4 * row, g);
    else
      for (int k = 0; k < 4; ++k) g[k] = nan4[k];
    ori_product(ops.q[s], g, e);
    double2 *dst = reinterpret_cast<double2 *>(S + ((size_t)s * rows + r) * 4);
    dst[0] = make_double2(e[0], e[1]);
    dst[1] = make_double2(e[2], e[3]);
  }
}

struct OuterArgs {
  const double *q1, *q2;  // [n][4], [m][4] raw rows
  int64_t n, m;
  int64_t row_first;      // first row of this pass
  int64_t pass_rows;      // rows of this pass
  int64_t tiles_j;
  OriOps ops1, ops2;
  double scale;
  void *out;              // [pass_rows][m] of T
};

template <typename T>
__global__ __launch_bounds__(ORI_THREADS) void orientation_outer_kernel(OuterArgs a) {
  __shared__ double As[ORI_MAX_OPS * ORI_TILE_I * 4];
  __shared__ double Bs[ORI_MAX_OPS * ORI_TILE_J * 4];
  __shared__ double Os[ORI_TILE_I * ORI_TILE_J];
  int64_t row0, col0;
  ori_tile_origin((int64_t)blockIdx.x, a.tiles_j, &row0, &col0);
  // rows of the pass past its end are staged as NaN too: `total` is the end of the pass, not of the set
  const int64_t row_end = a.row_first + a.pass_rows < a.n ? a.row_first + a.pass_rows : a.n;
  stage_equivalents(a.q1, a.row_first + row0, row_end, ORI_TILE_I, a.ops1, As);
  stage_equivalents(a.q2, col0, a.m, ORI_TILE_J, a.ops2, Bs);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wi = (wave >> 1) * ORI_MFMA, wj = (wave & 1) * ORI_MFMA, lo = lane & 15, lk = lane >> 4;
  const int n1 = a.ops1.n, n2 = a.ops2.n;
  double best[4] = {-1.0, -1.0, -1.0, -1.0};
  int at1[4] = {0, 0, 0, 0}, at2[4] = {0, 0, 0, 0};
  for (int s1 = 0; s1 < n1; ++s1) {
    const double av = As[((size_t)s1 * ORI_TILE_I + wi + lo) * 4 + lk];
    for (int s2 = 0; s2 < n2; ++s2) {
      const double bv = Bs[((size_t)s2 * ORI_TILE_J + wj + lo) * 4 + lk];
      const ori_d4 d = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, ori_d4{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double v = fabs(d[g]);
        const bool take = v > best[g];
        best[g] = take ? v : best[g];
        at1[g] = take ? s1 : at1[g];
        at2[g] = take ? s2 : at2[g];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int r = wi + lk + 4 * g, c = wj + lo;
    const double *e1 = As + ((size_t)at1[g] * ORI_TILE_I + r) * 4;
    const double *e2 = Bs + ((size_t)at2[g] * ORI_TILE_J + c) * 4;
    const double p1[4] = {e1[0], e1[1], e1[2], e1[3]}, p2[4] = {e2[0], e2[1], e2[2], e2[3]};
    Os[r * ORI_TILE_J + c] = ori_angle(p1, p2) * a.scale;
  }
  __syncthreads();
  // thread t: row t / 8 of the tile, its columns 4 (t % 8) ... + 3
  const int r = threadIdx.x / (ORI_TILE_J / 4), c = threadIdx.x % (ORI_TILE_J / 4) * 4;
  const int64_t row = row0 + r, col = col0 + c;
  if (row >= a.pass_rows || col >= a.m) return;
  struct Four {
    T v[4];
  };
  Four f;
#pragma unroll
  for (int e = 0; e < 4; ++e) f.v[e] = (T)Os[r * ORI_TILE_J + c + e];
  T *dst = reinterpret_cast<T *>(a.out) + ori_out_index(row, col, a.m);
  if (col + 4 <= a.m) {
    *reinterpret_cast<Four *>(dst) = f;
  } else {
    for (int e = 0; e < 4 && col + e < a.m; ++e) dst[e] = f.v[e];
  }
}

bool ops_refused(const OriOps &o) { return o.n < 1 || o.n > ORI_MAX_OPS; }

}  // namespace

hipError_t launch_orientation_pairs(const OriPairsLaunch &l, hipStream_t s) {
  if (!l.q1 || !l.q2 || !l.out || l.count < 1 || l.shape.nd < 0 || l.shape.nd > ORI_MAX_DIMS || ops_refused(l.ops1) ||
      ops_refused(l.ops2) || ori_blocks(l.count) > ORI_MAX_TILES)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(orientation_pairs_kernel, dim3((unsigned)ori_blocks(l.count)), dim3(ORI_THREADS), 0, s, l.q1, l.q2, l.shape,
                     l.count, l.ops1, l.ops2, l.degrees ? ORI_DEGREES : 1.0, l.out);
  return hipGetLastError();
}

hipError_t launch_orientation_outer(const OriOuterLaunch &l, hipStream_t s) {
  if (!l.q1 || !l.q2 || !l.out || l.n < 1 || l.m < 1 || l.row_first < 0 || l.pass_rows < 1 || l.row_first + l.pass_rows > l.n ||
      ops_refused(l.ops1) || ops_refused(l.ops2) || (l.elem_bytes != 4 && l.elem_bytes != 8))
    return hipErrorInvalidValue;
  OuterArgs a{};
  a.q1 = l.q1;
  a.q2 = l.q2;
  a.n = l.n;
  a.m = l.m;
  a.row_first = l.row_first;
  a.pass_rows = l.pass_rows;
  a.tiles_j = (l.m + ORI_TILE_J - 1) / ORI_TILE_J;
  a.ops1 = l.ops1;
  a.ops2 = l.ops2;
  a.scale = l.degrees ? ORI_DEGREES : 1.0;
  a.out = l.out;
  const int64_t tiles = (l.pass_rows + ORI_TILE_I - 1) / ORI_TILE_I * a.tiles_j;
  if (tiles > ORI_MAX_TILES) return hipErrorInvalidValue;
  if (l.elem_bytes == 8)
    hipLaunchKernelGGL(orientation_outer_kernel<double>, dim3((unsigned)tiles), dim3(ORI_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL(orientation_outer_kernel<float>, dim3((unsigned)tiles), dim3(ORI_THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_orientation_reduce(const OriReduceLaunch &l, hipStream_t s) {
  if (!l.q || !l.out || !l.index || l.n < 1 || ops_refused(l.ops) || ori_blocks(l.n) > ORI_MAX_TILES) return hipErrorInvalidValue;
  hipLaunchKernelGGL(orientation_reduce_kernel, dim3((unsigned)ori_blocks(l.n)), dim3(ORI_THREADS), 0, s, l.q, l.n, l.ops, l.out,
                     l.index);
  return hipGetLastError();
}

hipError_t launch_orientation_kam(const OriKamLaunch &l, hipStream_t s) {
  if (!l.rot || !l.out || l.ny < 1 || l.nx < 1 || ops_refused(l.ops) || l.n_offsets < 0 || l.n_offsets > ORI_MAX_OFFSETS ||
      (l.n_offsets > 0 && !l.offsets) || ori_blocks((int64_t)l.ny * l.nx) > ORI_MAX_TILES)
    return hipErrorInvalidValue;
  OriOps one{};
  one.n = 1;
  one.q[0][0] = 1.0;
  const int64_t points = (int64_t)l.ny * l.nx;
  hipLaunchKernelGGL(orientation_kam_kernel, dim3((unsigned)ori_blocks(points)), dim3(ORI_THREADS), 0, s, l.rot, l.ny, l.nx, one,
                     l.ops, l.offsets, l.n_offsets, l.in_data, l.max_angle, l.degrees ? ORI_DEGREES : 1.0, l.out);
  return hipGetLastError();
}

}  // namespace kpdi
