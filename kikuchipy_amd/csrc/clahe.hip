// clahe.hip - adaptive histogram equalization of every resident experimental pattern (EBSD.adaptive_histogram_equalization,
// signals/_kikuchipy_signal.py:340-470; pattern/_pattern.py:810-840), i.e. scikit-image 0.18.3's equalize_adapthist
// followed by kikuchipy's rescale_intensity(dtype_out=<dtype>), as NumPy 1.26 evaluates them:
//
//   1. img_as_uint: uint8 * 257; uint16 as is; int8 / int16 scaled (x * 16513 >> 5, x * 32769 >> 14, negatives 0);
//      floats clip(rint(x * 65535), 0, 65535) in the input's float type, then the x86-64 cast (NaN -> 0).
//   2. 14 bits: rint(((u - umin) / (umax - umin)) * 16383) in float64 (half to even); a constant image: min(u, 16383).
//   3. bins: v // (1 + 16384 // nbins).  The image is padded by numpy 'reflect' (k // 2 before, to a multiple of k plus
//      ceil(k / 2) after); tile (ty, tx) covers detector rows [ty ky, (ty + 1) ky) and columns alike, reflected.
//   4. per tile: the histogram, clip_histogram(clip_count) (integer-exact, the reference's redistribution loop), then
//      lut = min(trunc(cumsum * (16383.0 / (ky kx))), 16383).
//   5. per pixel: the four tables around its interpolation block (edge-padded), in np.ndindex(2, 2) order, each
//      float64 product lut * (wx * wy) rounded to float32 and added to a float32 sum from 0, truncated to uint16.
//   6. x = v * (1.0 / 65535), skimage's rescale_intensity to [0, 1] (identity for a constant image), kikuchipy's
//      ((x - xmin) / (xmax - xmin)) * (omax - omin) + omin in float64 with the dtype's range, then ndarray.astype
//      (integer dtypes: truncate to int32, NaN -> INT32_MIN, keep the low bits).
//
// Histograms count with atomics (LDS on path 0, global vector atomics on path 1); counting does not depend on the order,
// and everything else is per tile or per pixel, so both paths give the same bits.  Per-pattern minima / maxima are
// integer.  The library builds with -ffp-contract=off: no product is fused into a sum.  Paths: clahe_plan.h.
#include "../../include/kpdi.h"
#include "clahe_plan.h"
#include "kernels.h"

#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace kpdi {

namespace {

constexpr int CL_WAVES = CLAHE_THREADS / 64;

// img_as_uint (skimage 0.18.3 _convert) of one value
template <typename T>
__device__ __forceinline__ unsigned cl_to_u16(T x) {
  if constexpr (std::is_same<T, uint8_t>::value) {
    return (unsigned)x * 257u;
  } else if constexpr (std::is_same<T, uint16_t>::value) {
    return x;
  } else if constexpr (std::is_same<T, int8_t>::value) {
    const int t = ((int)x * 16513) >> 5;  // _scale(7 -> 16 bits): via 21 bits, floor division
    return t < 0 ? 0u : (unsigned)t;
  } else if constexpr (std::is_same<T, int16_t>::value) {
    const int t = ((int)x * 32769) >> 14;  // _scale(15 -> 16 bits): via 30 bits
    return t < 0 ? 0u : (unsigned)t;
  } else {
    T y = rint(x * (T)65535);  // np.multiply(image, 65535, dtype=<input float>), np.rint
    y = (y > (T)0 || y != y) ? y : (T)0;  // np.clip: NaN stays
    y = (y < (T)65535 || y != y) ? y : (T)65535;
    const int32_t i = (y == y) ? (int32_t)y : INT32_MIN;  // .astype(uint16) on x86-64
    return (unsigned)(uint16_t)(uint32_t)i;
  }
}

// ndarray.astype(TO) of a float64 result
template <typename TO>
__device__ __forceinline__ TO cl_cast(double y) {
  if constexpr (std::is_floating_point<TO>::value) {
    return (TO)y;
  } else {
    const int32_t i = (y >= -2147483648.0 && y < 2147483648.0) ? (int32_t)y : INT32_MIN;  // NaN: INT32_MIN
    return (TO)(uint32_t)i;
  }
}

__device__ __forceinline__ long long cl_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// block-wide integer min / max, every thread gets the result
__device__ __forceinline__ void cl_block_minmax(unsigned &mn, unsigned &mx, unsigned *red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = min(mn, (unsigned)__shfl_xor((int)mn, o, 64));
    mx = max(mx, (unsigned)__shfl_xor((int)mx, o, 64));
  }
  __syncthreads();  // `red` may still be read from the previous reduction
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = mn;
    red[CL_WAVES + (threadIdx.x >> 6)] = mx;
  }
  __syncthreads();
  mn = red[0];
  mx = red[CL_WAVES];
  for (int i = 1; i < CL_WAVES; ++i) {
    mn = min(mn, red[i]);
    mx = max(mx, red[CL_WAVES + i]);
  }
}

// clip_histogram (skimage 0.18.3) of one tile's histogram `h` (nbins counts) by one wave; lane l owns bins l, l + 64, ...
template <typename H>
__device__ void cl_clip(H *h, int nbins, int clim) {
  const int lane = threadIdx.x & 63;
  long long part = 0;
  for (int b = lane; b < nbins; b += 64) {
    const int v = (int)h[b];
    if (v > clim) {
      part += v - clim;
      h[b] = (unsigned)clim;
    }
  }
  long long n_excess = cl_wave_sum(part);
  const long long bin_incr = n_excess / nbins;  // n_excess >= 0
  const long long upper = clim - bin_incr;
  part = 0;
  for (int b = lane; b < nbins; b += 64) {
    const int v = (int)h[b];
    if (v < upper) {
      h[b] = (unsigned)(v + bin_incr);
      ++part;
    }
  }
  n_excess -= cl_wave_sum(part) * bin_incr;
  part = 0;
  for (int b = lane; b < nbins; b += 64) {  // mid_mask, on the histogram as it now is
    const int v = (int)h[b];
    if (v >= upper && v < clim) {
      part += v - clim;
      h[b] = (unsigned)clim;
    }
  }
  n_excess += cl_wave_sum(part);
  while (n_excess > 0) {  // redistribute what is left
    const long long prev = n_excess;
    for (int index = 0; index < nbins; ++index) {
      part = 0;
      for (int b = lane; b < nbins; b += 64) part += (int)h[b] < clim;
      const long long under = cl_wave_sum(part);
      if (under == 0) break;  // nothing can take more: this and every later index add nothing
      long long step = under / n_excess;
      if (step < 1) step = 1;
      part = 0;
      for (int b = lane; b < nbins; b += 64) {
        if (b >= index && (b - index) % step == 0 && (int)h[b] < clim) {
          h[b] = h[b] + 1u;
          ++part;
        }
      }
      n_excess -= cl_wave_sum(part);
      if (n_excess <= 0) break;
    }
    if (prev == n_excess) break;
  }
}

// map_histogram: lut[b] = min(trunc(cumsum(h)[b] * scale), 16383), one wave
template <typename H, typename L>
__device__ void cl_map(const H *h, L *lut, int nbins, double scale) {
  const int lane = threadIdx.x & 63;
  long long carry = 0;
  for (int base = 0; base < nbins; base += 64) {
    const int b = base + lane;
    long long incl = b < nbins ? (long long)(int)h[b] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (b < nbins) lut[b] = (uint16_t)(int)fmin((double)(carry + incl) * scale, 16383.0);
    carry += __shfl(incl, 63, 64);
  }
}

// the workspace path's global memory is shared between the workgroup's waves through L2: fence before each barrier
template <bool LDS>
__device__ __forceinline__ void cl_sync() {
  if constexpr (!LDS) __threadfence();
  __syncthreads();
}

__device__ __forceinline__ int cl_reflect(int j, int n) {  // numpy 'reflect' (no edge repeat), any distance
  if (j < n) return j;
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  const int m = j % period;
  return m < n ? m : period - m;
}

template <typename T, bool LDS>
__global__ __launch_bounds__(CLAHE_THREADS) void clahe_kernel(ClaheLaunch a, ClahePlan pl, int64_t first) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cl_lds[];
  __shared__ unsigned red[2 * CL_WAVES];
  const int sy = a.sy, sx = a.sx, ky = a.ky, kx = a.kx, nbins = a.nbins;
  const int nty = pl.nty, ntx = pl.ntx, tid = threadIdx.x;
  const int npix = sy * sx;
  const int ery = nty * ky, erx = ntx * kx;  // rows / columns of the histogrammed region
  const int64_t pat = first + blockIdx.x;
  T *p = (T *)a.patterns + pat * npix;

  // tables: per detector row / column the interpolation block and r / k; per region row / column source and tile
  double *wt = (double *)cl_lds;
  int *blk = (int *)(cl_lds + ((size_t)sy + sx) * sizeof(double));
  int *esrc = (int *)(cl_lds + clahe_align(((size_t)sy + sx) * 12));
  int *etile = esrc + ery + erx;
  unsigned char *rest = cl_lds + clahe_table_bytes(sy, sx, nty, ntx, ky, kx);
  for (int i = tid; i < sy + sx; i += CLAHE_THREADS) {
    const int k = i < sy ? ky : kx;
    const int j = (i < sy ? i : i - sy) + k / 2;  // the padded coordinate
    blk[i] = j / k;
    wt[i] = (double)(j % k) / (double)k;  // np.arange(k) / k
  }
  for (int i = tid; i < ery + erx; i += CLAHE_THREADS) {
    const bool row = i < ery;
    const int e = row ? i : i - ery, k = row ? ky : kx;
    esrc[i] = cl_reflect(e, row ? sy : sx);
    etile[i] = e / k;
  }

  uint16_t *bins, *res;
  unsigned *hist;
  uint16_t *lut;
  const size_t row_bins = (size_t)ntx * nbins;
  if constexpr (LDS) {
    bins = (uint16_t *)rest;
    res = bins;  // one band: every histogram is complete before the first result is written
    hist = (unsigned *)(rest + clahe_align((size_t)npix * 2));
    lut = (uint16_t *)((unsigned char *)hist + clahe_align((size_t)nty * row_bins * 4));
  } else {
    unsigned char *slot = (unsigned char *)a.workspace + (size_t)blockIdx.x * pl.slot_bytes;
    bins = (uint16_t *)slot;
    res = (uint16_t *)(slot + clahe_align((size_t)npix * 2));
    hist = (unsigned *)(slot + 2 * clahe_align((size_t)npix * 2));
    lut = (uint16_t *)((unsigned char *)hist + clahe_align(row_bins * pl.band * 4));
  }

  // 1. img_as_uint and its range
  unsigned mn = 0xffffffffu, mx = 0;
  for (int i = tid; i < npix; i += CLAHE_THREADS) {
    const unsigned u = cl_to_u16(p[i]);
    bins[i] = (uint16_t)u;
    mn = min(mn, u);
    mx = max(mx, u);
  }
  cl_block_minmax(mn, mx, red);
  // 2. 14 bits, then the bin
  {
    const double imin = (double)mn, span = (double)mx - (double)mn;
    const int bin_size = 1 + 16384 / nbins;
    for (int i = tid; i < npix; i += CLAHE_THREADS) {
      const unsigned u = bins[i];
      const unsigned v = mn != mx ? (unsigned)rint((((double)u - imin) / span) * 16383.0 + 0.0) : min(u, 16383u);
      bins[i] = (uint16_t)(v / bin_size);
    }
  }
  cl_sync<LDS>();

  const int kk = ky * kx;
  const double scale = 16383.0 / (double)kk;
  const int ring = pl.band == nty ? nty : pl.band + 1;  // rows of tables kept: the band's and the one before
  const int wave = tid >> 6;
  const int rowstep = CLAHE_THREADS / erx, colstep = CLAHE_THREADS % erx;
  const int orowstep = CLAHE_THREADS / sx, ocolstep = CLAHE_THREADS % sx;
  unsigned vmin = 0xffffffffu, vmax = 0;
  for (int t0 = 0; t0 < nty; t0 += pl.band) {
    const int t1 = min(t0 + pl.band, nty), nb = t1 - t0;
    for (size_t i = tid; i < (size_t)nb * row_bins; i += CLAHE_THREADS) hist[i] = 0;
    cl_sync<LDS>();
    // 3. histograms of tile rows [t0, t1): region rows [t0 ky, t1 ky), every region column
    {
      int r = tid / erx, c = tid % erx;
      const int rows = nb * ky;
      while (r < rows) {
        const int er = t0 * ky + r;
        const int b = bins[esrc[er] * sx + esrc[ery + c]];
        atomicAdd(&hist[((size_t)(etile[er] - t0) * ntx + etile[ery + c]) * nbins + b], 1u);
        c += colstep;
        r += rowstep;
        if (c >= erx) {
          c -= erx;
          ++r;
        }
      }
    }
    cl_sync<LDS>();
    // 4. clip and map, one wave per tile
    for (int t = wave; t < nb * ntx; t += CL_WAVES) {
      unsigned *h = hist + (size_t)t * nbins;
      const int ty = t0 + t / ntx, tx = t % ntx;
      if (a.clip_count < kk) cl_clip(h, nbins, a.clip_count);
      cl_map(h, lut + ((size_t)(ty % ring) * ntx + tx) * nbins, nbins, scale);
    }
    cl_sync<LDS>();
    // 5. the interpolation blocks whose tables are all known: block rows [t0, t1), and the last one after the last band
    {
      const int bend = t1 < nty ? t1 : nty + 1;
      const int r0 = (int)max((int64_t)0, (int64_t)t0 * ky - ky / 2);
      const int r1 = (int)min((int64_t)sy, (int64_t)bend * ky - ky / 2);
      int r = r0 + tid / sx, c = tid % sx;
      while (r < r1) {
        const int by = blk[r], bx = blk[sy + c];
        const double wy1 = wt[r], wx1 = wt[sy + c];
        const double wy0 = 1.0 - wy1, wx0 = 1.0 - wx1;
        const int ty0 = (max(by - 1, 0) % ring) * ntx, ty1 = (min(by, nty - 1) % ring) * ntx;
        const int tx0 = max(bx - 1, 0), tx1 = min(bx, ntx - 1);
        const int i = r * sx + c;
        const int b = bins[i];
        float acc = 0.0f;
        acc += (float)((double)lut[((size_t)ty0 + tx0) * nbins + b] * (wx0 * wy0));
        acc += (float)((double)lut[((size_t)ty0 + tx1) * nbins + b] * (wx1 * wy0));
        acc += (float)((double)lut[((size_t)ty1 + tx0) * nbins + b] * (wx0 * wy1));
        acc += (float)((double)lut[((size_t)ty1 + tx1) * nbins + b] * (wx1 * wy1));
        const unsigned v = (unsigned)acc;
        res[i] = (uint16_t)v;
        vmin = min(vmin, v);
        vmax = max(vmax, v);
        c += ocolstep;
        r += orowstep;
        if (c >= sx) {
          c -= sx;
          ++r;
        }
      }
    }
    cl_sync<LDS>();
  }
  cl_block_minmax(vmin, vmax, red);

  // 6. img_as_float, skimage's rescale to [0, 1], kikuchipy's rescale to the dtype's range, the cast
  const double c = 1.0 / 65535.0;
  const double xa = (double)vmin * c, xb = (double)vmax * c;
  auto x2 = [&](unsigned v) {
    const double x = (double)v * c;
    return xa != xb ? ((x - xa) / (xb - xa)) * 1.0 + 0.0 : x;
  };
  const double m = x2(vmin), range = x2(vmax) - m;
  const double omin = a.omin, orange = a.omax - a.omin;
  for (int i = tid; i < npix; i += CLAHE_THREADS) p[i] = cl_cast<T>(((x2(res[i]) - m) / range) * orange + omin);
}

template <typename T>
hipError_t launch_clahe_t(const ClaheLaunch &a, const ClahePlan &pl, hipStream_t s) {
  if (pl.path == 0) {
    hipError_t e = hipFuncSetAttribute((const void *)clahe_kernel<T, true>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)CLAHE_LDS_CAP);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((clahe_kernel<T, true>), dim3((unsigned)a.n), dim3(CLAHE_THREADS), pl.lds_bytes, s, a, pl,
                       (int64_t)0);
    return hipGetLastError();
  }
  hipError_t e = hipFuncSetAttribute((const void *)clahe_kernel<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)CLAHE_TABLE_CAP);
  if (e != hipSuccess) return e;
  for (int64_t first = 0; first < a.n; first += pl.per_launch) {
    const int64_t cnt = a.n - first < pl.per_launch ? a.n - first : pl.per_launch;
    hipLaunchKernelGGL((clahe_kernel<T, false>), dim3((unsigned)cnt), dim3(CLAHE_THREADS), pl.lds_bytes, s, a, pl,
                       first);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

ClahePlan clahe_launch_plan(int dtype, int sy, int sx, int ky, int kx, int nbins, int64_t n) {
  bool force = false;
  if (const char *e = getenv("KPDI_CLAHE_PATH")) force = atoi(e) == 1;  // tests: path 1 for any shape
  return clahe_plan(dtype, sy, sx, ky, kx, nbins, n, force);
}

hipError_t launch_clahe(const ClaheLaunch &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const ClahePlan pl = clahe_launch_plan(a.dtype, a.sy, a.sx, a.ky, a.kx, a.nbins, a.n);
  if (pl.path < 0 || !a.patterns || a.clip_count < 1) return hipErrorInvalidValue;
  if (pl.path == 1 && (!a.workspace || a.workspace_bytes < pl.workspace_bytes)) return hipErrorInvalidValue;
  return with_pattern_type(a.dtype, [&](auto t) { return launch_clahe_t<decltype(t)>(a, pl, s); });
}

}  // namespace kpdi
