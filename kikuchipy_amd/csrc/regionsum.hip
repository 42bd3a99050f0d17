// regionsum.hip - sums of every resident pattern over a list of detector rectangles (EBSD.get_virtual_bse_intensity,
// signals/ebsd.py:1555-1598 and :3091-3105; imaging/vbse.py:239-283 reads them for a whole grid):
//   sums[i][k] = nansum(p_i[row0_k:row1_k, col0_k:col1_k]).
// The patterns are read from device memory once, whatever the number of rectangles: a wave stages a block of whole rows
// in LDS with 16-byte loads (regionsum_plan.h: a 60 x 60 uint8 pattern is one block, four patterns per workgroup) and
// all rectangles are then summed out of LDS.  RS_GROUP lanes share a rectangle: the part of it inside the block is cut,
// row by row, into pieces of RS_PIECE pixels, lane j adds the pieces j, j + 16, ... in that order in a register and the
// 16 lanes are combined by the xor butterfly 8 ... 1 (the wave stage of pattern_dft.h's block_reduce on 16 lanes).
// Blocks of one pattern are added in block order by a second kernel.  No atomics: the order of every sum is a function
// of dtype, shape and the rectangle alone.
// Arithmetic: unsigned patterns in uint64, signed ones in int64 (pieces in 32 bits: 16 x 2^16 fits), exact; float
// patterns in float64 with NaN counted as 0 (inf + -inf gives NaN as np.nansum does), rounded once to the output.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "regionsum_plan.h"

namespace kpdi {

namespace {

typedef uint32_t rs_chunk __attribute__((ext_vector_type(4)));  // 16 bytes, one load

template <typename T> struct RsType { using Acc = unsigned long long; using Piece = uint32_t; using Out = unsigned long long; };
template <> struct RsType<int8_t> { using Acc = long long; using Piece = int32_t; using Out = long long; };
template <> struct RsType<int16_t> { using Acc = long long; using Piece = int32_t; using Out = long long; };
template <> struct RsType<float> { using Acc = double; using Piece = double; using Out = float; };
template <> struct RsType<double> { using Acc = double; using Piece = double; using Out = double; };

template <typename T>
__device__ __forceinline__ typename RsType<T>::Piece rs_value(T v) {
  if constexpr (std::is_floating_point<T>::value) return v != v ? 0.0 : (double)v;
  else return (typename RsType<T>::Piece)v;
}

// `all`: the whole resident set of n_all patterns (what may be loaded); this launch takes the blocks of the patterns
// first ... first + n.  Dst: the output type (path 0) or the accumulator (path 1: partial sums [pattern][block][rect]).
template <typename T, typename Dst>
__global__ __launch_bounds__(RS_THREADS) void region_sums_kernel(const T *__restrict__ all, int64_t n_all, int64_t first, int64_t n,
                                                                int sy, int sx, int rb, int nblk, int slot,
                                                                const int4 *__restrict__ rects, int n_rects,
                                                                Dst *__restrict__ dst) {
  using Acc = typename RsType<T>::Acc;
  using Piece = typename RsType<T>::Piece;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int4 *rtab = (int4 *)smem;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  char *buf = smem + RS_RECT_TILE * sizeof(int4) + (size_t)w * slot;
  const int64_t unit = (int64_t)blockIdx.x * RS_WAVES + w;
  const bool valid = unit < n * nblk;  // (wave-uniform; a wave without a block still takes part in the barriers)
  int y0 = 0, nrows = 0;
  const T *img = nullptr;  // the block's first pixel in LDS
  if (valid) {
    const int64_t pat = unit / nblk;
    y0 = (int)(unit - pat * nblk) * rb;
    nrows = min(rb, sy - y0);
    const uintptr_t base = (uintptr_t)all, end = base + (size_t)n_all * sy * sx * sizeof(T);
    const uintptr_t a = base + ((size_t)(first + pat) * sy * sx + (size_t)y0 * sx) * sizeof(T);
    const uintptr_t a0 = a & ~(uintptr_t)15, a1 = (a + (size_t)nrows * sx * sizeof(T) + 15) & ~(uintptr_t)15;
    img = (const T *)(buf + (a - a0));
    const int nchunks = (int)((a1 - a0) >> 4);  // <= slot / 16 (regionsum_plan.h)
    for (int c = lane; c < nchunks; c += 64) {
      const uintptr_t g = a0 + (uintptr_t)c * 16;
      if (g >= base && g + 16 <= end) {
        *(rs_chunk *)(buf + c * 16) = __builtin_nontemporal_load((const rs_chunk *)g);
      } else {  // the chunk reaches over an end of the resident set: only the bytes inside it
        for (int b = 0; b < 16; ++b)
          if (g + b >= base && g + b < end) buf[c * 16 + b] = *(const char *)(g + b);
      }
    }
  }
  for (int t0 = 0; t0 < n_rects; t0 += RS_RECT_TILE) {
    const int tn = min(RS_RECT_TILE, n_rects - t0);
    __syncthreads();  // the block is in LDS; the previous tile of bounds is read
    for (int i = threadIdx.x; i < tn; i += RS_THREADS) rtab[i] = rects[t0 + i];
    __syncthreads();
    if (!valid) continue;
    for (int p = 0; p < tn; p += 64 / RS_GROUP) {
      const int k = p + lane / RS_GROUP, j = lane % RS_GROUP;
      Acc s = 0;
      if (k < tn) {
        const int4 r = rtab[k];  // (row0, row1, col0, col1)
        const int ra = max(r.x, y0), re = min(r.y, y0 + nrows), nc = r.w - r.z;
        if (ra < re && nc > 0) {
          const int ipr = (nc + RS_PIECE - 1) / RS_PIECE, items = (re - ra) * ipr;
          int row = j / ipr, piece = j - row * ipr;
          for (int t = j; t < items; t += RS_GROUP) {
            const int c0 = r.z + piece * RS_PIECE, c1 = min(r.w, c0 + RS_PIECE);
            const T *e = img + (ra - y0 + row) * sx;
            if constexpr (std::is_floating_point<T>::value) {
              for (int x = c0; x < c1; ++x) s += rs_value(e[x]);
            } else {
              Piece ps = 0;
              for (int x = c0; x < c1; ++x) ps += rs_value(e[x]);
              s += (Acc)ps;
            }
            piece += RS_GROUP;
            while (piece >= ipr) {
              piece -= ipr;
              ++row;
            }
          }
        }
      }
#pragma unroll
      for (int o = RS_GROUP / 2; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      if (k < tn && j == 0) dst[unit * n_rects + t0 + k] = (Dst)s;
    }
  }
}

// path 1: the blocks of a pattern in block order
template <typename Acc, typename Out>
__global__ void region_sums_final_kernel(const Acc *__restrict__ partial, int64_t count, int nblk, int n_rects, Out *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t pat = i / n_rects, k = i - pat * n_rects;
  Acc s = 0;
  for (int b = 0; b < nblk; ++b) s += partial[(pat * nblk + b) * n_rects + k];
  out[i] = (Out)s;
}

template <typename T>
hipError_t launch_rs_t(const RsLaunch &a, const RsPlan &plan, hipStream_t s) {
  using Acc = typename RsType<T>::Acc;
  using Out = typename RsType<T>::Out;
  const T *pats = (const T *)a.patterns;
  const int4 *rects = (const int4 *)a.rects;
  Out *out = (Out *)a.out;
  const int nblk = plan.blocks_per_pattern;
  auto grid = [&](int64_t b) { return dim3((unsigned)((b * nblk + RS_WAVES - 1) / RS_WAVES)); };
  if (plan.path == 0) {
    hipLaunchKernelGGL((region_sums_kernel<T, Out>), grid(a.n), dim3(RS_THREADS), plan.lds_bytes, s, pats, a.n, (int64_t)0, a.n,
                       a.sy, a.sx, plan.rows_per_block, nblk, (int)plan.slot_bytes, rects, a.n_rects, out);
    return hipGetLastError();
  }
  if (!a.workspace || a.workspace_bytes < plan.workspace_bytes) return hipErrorInvalidValue;
  Acc *partial = (Acc *)a.workspace;
  for (int64_t start = 0; start < a.n; start += plan.batch) {
    const int64_t b = std::min<int64_t>(plan.batch, a.n - start), count = b * a.n_rects;
    hipLaunchKernelGGL((region_sums_kernel<T, Acc>), grid(b), dim3(RS_THREADS), plan.lds_bytes, s, pats, a.n, start, b, a.sy,
                       a.sx, plan.rows_per_block, nblk, (int)plan.slot_bytes, rects, a.n_rects, partial);
    hipLaunchKernelGGL((region_sums_final_kernel<Acc, Out>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, partial,
                       count, nblk, a.n_rects, out + start * a.n_rects);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

hipError_t launch_region_sums(const RsLaunch &a, hipStream_t s) {
  if (a.n <= 0 || a.n_rects <= 0) return hipSuccess;
  const RsPlan plan = rs_plan(a.dtype, a.sy, a.sx, a.n, a.n_rects);
  if (plan.path < 0 || plan.batch * plan.blocks_per_pattern / RS_WAVES >= (int64_t)INT32_MAX ||
      plan.batch * a.n_rects / 256 >= (int64_t)INT32_MAX)
    return hipErrorInvalidValue;
  return with_pattern_type(a.dtype, [&](auto t) { return launch_rs_t<decltype(t)>(a, plan, s); });
}

}  // namespace kpdi
