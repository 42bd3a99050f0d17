// downsample.hip - binning of every resident experimental pattern by an integer factor, rescaled to the range of the
// output dtype (EBSD.downsample, signals/ebsd.py:1113-1219; _bin2d / _downsample2d, pattern/_pattern.py:776-807), with the
// reference's arithmetic as NumPy 1.26 evaluates its py_func:
//
//   p = float32(pattern)
//   b[r, c] = float32 sum of p[r f + rr, c f + cc], added one by one from 0, rr outer and cc inner
//   imin, imax = np.min(b), np.max(b)                      (float32; NaN propagates)
//   (b - imin) / float32(imax - imin) * (omax - omin) + omin   (rescale() of prep_device.h: every operation rounded to
//                                                           float32, IEEE division, no contraction: -ffp-contract=off)
//   .astype(dtype_out)                                     (astype_cast of prep_device.h)
//
// One workgroup per pattern, one pass over HBM.  A lane owns the binned pixels o, o + threads, ... and adds each one's
// source pixels in the order above, so every sum has the reference's bits whatever the launch looks like; min / max are
// exact operations, so the shared fixed-tree block_reduce gives np.min / np.max once a NaN flag is reduced with them
// (fminf / fmaxf skip NaN, np.min / np.max do not).  The binned image waits in LDS (path 0) or in a device workspace
// (path 1) between the binning pass and the rescale-and-store pass; each lane reads back only what it wrote.  Where the
// raw pattern fits into LDS beside the binned image it is brought in with 16-byte loads first and binned from there.
// No atomics.  Which path takes a shape: downsample_plan.h.
#include "../../include/kpdi.h"
#include "downsample_plan.h"
#include "kernels.h"
#include "pattern_dft.h"
#include "prep_device.h"

#include <cmath>
#include <cstdlib>

namespace kpdi {

namespace {

struct DsArgs {
  const void *src;
  void *dst;
  int64_t n;
  int sy, sx, factor, dtype_out;
  float omin, orange;
  int staged, in_lds;
  unsigned raw_bytes;  // staged: the binned image's offset in LDS
  float *workspace;    // path 1: [gridDim.x][nout]
};

template <typename TO>
__device__ __forceinline__ void ds_store(const float *b, TO *o, int nout, int threads, float imin, float irange, float orange,
                                         float omin) {
  for (int i = threadIdx.x; i < nout; i += threads) o[i] = astype_cast<TO>(rescale(b[i], imin, irange, orange, omin));
}

template <typename T, int THREADS>
__global__ __launch_bounds__(THREADS) void downsample_kernel(DsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ds_lds[];
  __shared__ double red[3 * (THREADS / 64)];
  const int f = a.factor, sx = a.sx, nx = sx / f, ny = a.sy / f, nout = ny * nx, npix = a.sy * sx;
  float *b = a.in_lds ? (float *)(ds_lds + a.raw_bytes) : a.workspace + (size_t)blockIdx.x * nout;
  for (int64_t pat = blockIdx.x; pat < a.n; pat += gridDim.x) {
    const T *p = (const T *)a.src + pat * npix;
    if (a.staged) {
      // the pattern's bytes into LDS: 16-byte words where its size allows them (its start is then aligned)
      const size_t bytes = (size_t)npix * sizeof(T);
      const unsigned char *g = (const unsigned char *)p;
      if ((bytes & 15) == 0) {
        for (size_t i = threadIdx.x; i < bytes / 16; i += THREADS)
          reinterpret_cast<uint4 *>(ds_lds)[i] = reinterpret_cast<const uint4 *>(g)[i];
      } else if ((bytes & 3) == 0) {
        for (size_t i = threadIdx.x; i < bytes / 4; i += THREADS)
          reinterpret_cast<uint32_t *>(ds_lds)[i] = reinterpret_cast<const uint32_t *>(g)[i];
      } else {
        for (size_t i = threadIdx.x; i < bytes; i += THREADS) ds_lds[i] = g[i];
      }
      __syncthreads();
      p = (const T *)ds_lds;
    }
    float mn = __builtin_inff(), mx = -__builtin_inff();
    int bad = 0;
    for (int o = threadIdx.x; o < nout; o += THREADS) {
      const int r = o / nx, c = o - r * nx;
      const T *q = p + (size_t)r * f * sx + c * f;
      float s = 0.f;
      for (int rr = 0; rr < f; ++rr, q += sx)
        for (int cc = 0; cc < f; ++cc) s += (float)q[cc];
      b[o] = s;
      mn = fminf(mn, s);
      mx = fmaxf(mx, s);
      bad |= s != s;
    }
    block_reduce<THREADS / 64, RedMin, RedMax, RedOr>(red, mn, mx, bad);
    if (bad) mn = mx = __builtin_nanf("");  // np.min / np.max of an image holding a NaN
    const float irange = mx - mn;
    const int64_t off = pat * nout;
    switch (a.dtype_out) {
      case KPDI_U8: ds_store(b, (uint8_t *)a.dst + off, nout, THREADS, mn, irange, a.orange, a.omin); break;
      case KPDI_I8: ds_store(b, (int8_t *)a.dst + off, nout, THREADS, mn, irange, a.orange, a.omin); break;
      case KPDI_U16: ds_store(b, (uint16_t *)a.dst + off, nout, THREADS, mn, irange, a.orange, a.omin); break;
      case KPDI_I16: ds_store(b, (int16_t *)a.dst + off, nout, THREADS, mn, irange, a.orange, a.omin); break;
      case KPDI_F32: ds_store(b, (float *)a.dst + off, nout, THREADS, mn, irange, a.orange, a.omin); break;
      case KPDI_F64: ds_store(b, (double *)a.dst + off, nout, THREADS, mn, irange, a.orange, a.omin); break;
      default: break;
    }
    __syncthreads();  // the staged pattern is overwritten by the next one
  }
}

template <typename T>
hipError_t launch_ds_t(const DsArgs &a, const DsPlan &plan, hipStream_t s) {
  if (plan.threads == 64)
    hipLaunchKernelGGL((downsample_kernel<T, 64>), dim3((unsigned)plan.grid), dim3(64), plan.lds_bytes, s, a);
  else
    hipLaunchKernelGGL((downsample_kernel<T, DS_THREADS>), dim3((unsigned)plan.grid), dim3(DS_THREADS), plan.lds_bytes, s, a);
  return hipGetLastError();
}

}  // namespace

DsPlan downsample_launch_plan(int dtype, int sy, int sx, int factor, int64_t n) {
  bool force = false;
  if (const char *e = getenv("KPDI_DOWNSAMPLE_PATH")) force = atoi(e) == 1;  // tests: path 1 for any shape
  return ds_plan(dtype, sy, sx, factor, n, force);
}

hipError_t launch_downsample(const DsLaunch &l, hipStream_t s) {
  if (l.n <= 0) return hipSuccess;
  const DsPlan plan = downsample_launch_plan(l.dtype, l.sy, l.sx, l.factor, l.n);
  if (plan.path < 0 || pattern_dtype_bytes(l.dtype_out) == 0 || !l.src || !l.dst || l.dst == l.src) return hipErrorInvalidValue;
  if (plan.path == 1 && (!l.workspace || l.workspace_bytes < plan.workspace_bytes)) return hipErrorInvalidValue;
  DsArgs a{};
  a.src = l.src;
  a.dst = l.dst;
  a.n = l.n;
  a.sy = l.sy;
  a.sx = l.sx;
  a.factor = l.factor;
  a.dtype_out = l.dtype_out;
  a.omin = l.omin;
  a.orange = l.omax - l.omin;
  a.staged = plan.path == 0 && plan.staged;
  a.in_lds = plan.path == 0;
  a.raw_bytes = (unsigned)plan.raw_bytes;
  a.workspace = (float *)l.workspace;
  return with_pattern_type(l.dtype, [&](auto t) { return launch_ds_t<decltype(t)>(a, plan, s); });
}

}  // namespace kpdi
