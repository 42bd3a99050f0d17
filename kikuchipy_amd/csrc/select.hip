// select.hip - a selection of the resident experimental patterns (EBSD.inav / isig / crop / extract_grid, deepcopy):
//
//   out[i, r, c] = in[index[i], row0 + r * row_step, col0 + c * col_step]
//
// for the element sizes 1, 2, 4 and 8: a byte-exact gather, bound by HBM.  Which of the three paths takes a selection,
// and the launch geometry: select_plan.h.
//   paths 0 / 1 (select_runs_kernel): the source is runs of contiguous bytes (one per pattern / one per output row).  A
//     lane owns one 16-byte piece of the output, aligned in the destination, so consecutive lanes store consecutive 16
//     bytes.  Its source address has whatever alignment the rectangle gives it: the piece is loaded as one, two, four,
//     eight or sixteen naturally aligned values (the alignment is the same for every piece of a run, so a wave takes one
//     branch per run).  Pieces cut by an end of the pattern's output or by the end of a run are moved byte by byte by
//     the lane that owns them.  Every output byte belongs to exactly one (pattern, piece) pair: it is written once, and
//     nothing outside [0, n_out * out_bytes) of the destination or outside the chosen pattern of the source is touched.
//   path 2 (select_strided_kernel): one element per lane.
// Offsets inside one pattern are 32-bit (select_plan.h refuses patterns of 2 GiB), every offset into a buffer is int64.
// No atomics, no LDS, no synchronisation.
#include "../../include/kpdi.h"
#include "kernels.h"
#include "select_plan.h"

namespace kpdi {

namespace {

struct SelArgs {
  const unsigned char *src;
  unsigned char *dst;
  const int64_t *index;       // [n_out] source pattern per output pattern, or nullptr (identity)
  int64_t n_out;
  int64_t src_pattern_bytes;  // sy * sx * esize
  unsigned out_bytes, run_bytes, items, ppb;
  unsigned first;             // of (row0, col0) in its pattern: bytes (paths 0 / 1), elements (path 2)
  unsigned row_pitch;         // between the starts of two output rows in the source: bytes / elements
  unsigned n_cols, col_step;  // path 2
};

// this lane's output pattern slot in the workgroup's group and its item in that pattern; false: the lane has none
__device__ __forceinline__ bool sel_item(const SelArgs &a, unsigned *slot, unsigned *item) {
  if (a.ppb > 1) {
    *slot = threadIdx.x / a.items;
    *item = threadIdx.x - *slot * a.items;
    return *slot < a.ppb;
  }
  *slot = 0;
  *item = blockIdx.x * SEL_THREADS + threadIdx.x;
  return *item < a.items;
}

// 16 bytes from an address of any alignment, as naturally aligned loads
__device__ __forceinline__ uint4 sel_load16(const unsigned char *p) {
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

template <bool WHOLE>
__global__ __launch_bounds__(SEL_THREADS) void select_runs_kernel(SelArgs a) {
  unsigned slot, item;
  if (!sel_item(a, &slot, &item)) return;
  for (int64_t g = blockIdx.y;; g += gridDim.y) {
    const int64_t i = g * a.ppb + slot;
    if (i >= a.n_out) break;
    const int64_t lo = i * (int64_t)a.out_bytes, hi = lo + a.out_bytes;
    const int64_t piece = (lo & ~(int64_t)(SEL_PIECE - 1)) + (int64_t)item * SEL_PIECE;
    if (piece >= hi) continue;  // (this pattern's output ends before the lane's piece)
    const int64_t b0 = piece > lo ? piece : lo, b1 = piece + SEL_PIECE < hi ? piece + SEL_PIECE : hi;
    const int64_t pat = a.index ? a.index[i] : i;
    const unsigned char *s = a.src + pat * a.src_pattern_bytes + a.first;
    const unsigned o = (unsigned)(b0 - lo);  // first output byte of the lane in its pattern
    unsigned run = WHOLE ? 0u : o / a.run_bytes, in = o - run * a.run_bytes;
    const unsigned char *sp = s + (size_t)run * a.row_pitch + in;
    const unsigned n = (unsigned)(b1 - b0);
    if (n == SEL_PIECE && (WHOLE || in + SEL_PIECE <= a.run_bytes)) {
      *reinterpret_cast<uint4 *>(a.dst + piece) = sel_load16(sp);
    } else {
      unsigned char *d = a.dst + b0;
      for (unsigned k = 0; k < n; ++k) {
        d[k] = *sp++;
        if (!WHOLE && ++in == a.run_bytes) {
          in = 0;
          ++run;
          sp = s + (size_t)run * a.row_pitch;  // (only dereferenced while k + 1 < n: an output byte of run `run`)
        }
      }
    }
  }
}

template <typename E>
__global__ __launch_bounds__(SEL_THREADS) void select_strided_kernel(SelArgs a) {
  unsigned slot, item;
  if (!sel_item(a, &slot, &item)) return;
  const unsigned r = item / a.n_cols, c = item - r * a.n_cols;
  const unsigned off = a.first + r * a.row_pitch + c * a.col_step;  // element of the source pattern
  const E *src = reinterpret_cast<const E *>(a.src);
  E *dst = reinterpret_cast<E *>(a.dst);
  const int64_t src_pattern = a.src_pattern_bytes / (int64_t)sizeof(E);
  for (int64_t g = blockIdx.y;; g += gridDim.y) {
    const int64_t i = g * a.ppb + slot;
    if (i >= a.n_out) break;
    const int64_t pat = a.index ? a.index[i] : i;
    dst[i * (int64_t)a.items + item] = src[pat * src_pattern + off];
  }
}

}  // namespace

hipError_t launch_select(const SelLaunch &l, hipStream_t s) {
  const SelPlan p = select_plan(l.esize, l.sy, l.sx, l.n_out, l.row0, l.row_step, l.n_rows, l.col0, l.col_step, l.n_cols);
  if (p.path < 0 || !l.src || !l.dst || l.src == l.dst) return hipErrorInvalidValue;
  SelArgs a{};
  a.src = (const unsigned char *)l.src;
  a.dst = (unsigned char *)l.dst;
  a.index = l.index;
  a.n_out = l.n_out;
  a.src_pattern_bytes = (int64_t)l.sy * l.sx * l.esize;
  a.out_bytes = p.out_bytes;
  a.run_bytes = p.run_bytes;
  a.items = p.items;
  a.ppb = p.patterns_per_block;
  const unsigned unit = p.path == SEL_STRIDED ? 1u : (unsigned)l.esize;
  a.first = ((unsigned)l.row0 * (unsigned)l.sx + (unsigned)l.col0) * unit;
  a.row_pitch = (unsigned)l.row_step * (unsigned)l.sx * unit;
  a.n_cols = (unsigned)l.n_cols;
  a.col_step = (unsigned)l.col_step;
  const dim3 grid(p.grid_x, p.grid_y), block(SEL_THREADS);
  if (p.path == SEL_WHOLE) {
    hipLaunchKernelGGL(select_runs_kernel<true>, grid, block, 0, s, a);
  } else if (p.path == SEL_ROWS) {
    hipLaunchKernelGGL(select_runs_kernel<false>, grid, block, 0, s, a);
  } else {
    switch (l.esize) {
      case 1: hipLaunchKernelGGL(select_strided_kernel<uint8_t>, grid, block, 0, s, a); break;
      case 2: hipLaunchKernelGGL(select_strided_kernel<uint16_t>, grid, block, 0, s, a); break;
      case 4: hipLaunchKernelGGL(select_strided_kernel<uint32_t>, grid, block, 0, s, a); break;
      default: hipLaunchKernelGGL(select_strided_kernel<uint64_t>, grid, block, 0, s, a); break;
    }
  }
  return hipGetLastError();
}

}  // namespace kpdi
