// hough_plan.h - the geometry of the Radon transform and of the band detection of Hough indexing (hough.hip), what one
// sinogram cell and one band compute, and how the work is laid on the chip: pure functions, no HIP call,
// `__host__ __device__` under hipcc and plain inline functions under a host compiler (tests/test_host_hough.py compiles
// this header with the host compiler).  Definitions: DESIGN.md section 26.
//
// A pattern of ny x nx pixels, centre cx = (nx - 1) / 2, cy = (ny - 1) / 2, is masked by its inscribed circle of radius
// R = (min(ny, nx) - 1) / 2 and the mean of the masked pixels is removed: the staged pattern, float32, 0 outside the mask.
// The sinogram S[a][k], a < n_theta, k < n_rho, is the sum of the staged pattern, sampled bilinearly at unit steps t along
// the line cos(theta) (j - cx) + sin(theta) (i - cy) = rho with theta = a pi / n_theta, rho = (k - (n_rho - 1) / 2) drho,
// drho = 2 floor(R) / (n_rho - 1) pixels, over the steps with rho^2 + t^2 <= R^2, t ascending, in float32 with every
// multiplication and addition rounded on its own (-ffp-contract=off).  cos and sin come from the host as float32 tables.
// Because theta + pi is the same line with -rho, S(a + n_theta, k) = S(a, n_rho - 1 - k): the theta seam.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HOUGH_HD __host__ __device__ inline
#else
#define HOUGH_HD inline
#endif

namespace kpdi {

constexpr int HOUGH_THREADS = 256;              // per workgroup of the Radon and the band kernel (4 waves)
constexpr size_t HOUGH_LDS_BYTES = 160 * 1024;  // LDS of a gfx950 CU, all of which one workgroup may ask for
constexpr size_t HOUGH_LDS_SCRATCH = HOUGH_THREADS * sizeof(double);  // the partial sums of the masked mean
constexpr int HOUGH_MAX_BANDS = 16;
constexpr int HOUGH_MAX_TAPS = 33;              // taps of one smoothing axis (radius 16)
constexpr int HOUGH_WINDOW = 3;                 // half width, in cells, of the window a local maximum dominates
constexpr int HOUGH_MAX_DIM = 4096;             // pixels along a detector axis, cells along a sinogram axis

struct HoughGeom {
  int ny, nx, n_theta, n_rho;
  int t_half;   // steps t = -t_half ... t_half
  int n_mask;   // pixels inside the mask
  float cx, cy, r2, drho, dtheta;
};

// one detected band: 32 bytes
struct HoughBand {
  float theta, rho;  // sub-cell position: radians, pixels
  float value;       // the smoothed sinogram at the cell
  int32_t valid;
  int32_t a, k;      // the cell
  float da, dk;      // sub-cell offsets in cells, each in [-0.5, 0.5]
};

struct HoughSmooth {
  int rt, rr;  // radii of the theta and the rho taps
  float wt[HOUGH_MAX_TAPS], wr[HOUGH_MAX_TAPS];
  int rim;     // cells at either end of the rho axis that hold no band
};

HOUGH_HD bool hough_in_mask(const HoughGeom &g, int i, int j) {
  const float dx = (float)j - g.cx, dy = (float)i - g.cy;
  return dx * dx + dy * dy <= g.r2;
}

// the default number of rho cells: one pixel per cell
HOUGH_HD int hough_default_n_rho(int ny, int nx) { return 2 * (((ny < nx ? ny : nx) - 1) / 2) + 1; }

inline HoughGeom hough_geom(int ny, int nx, int n_theta, int n_rho) {
  HoughGeom g{};
  g.ny = ny;
  g.nx = nx;
  g.n_theta = n_theta;
  g.n_rho = n_rho;
  const double r = ((ny < nx ? ny : nx) - 1) / 2.0;
  g.t_half = (int)std::ceil(r);
  g.cx = (float)((nx - 1) / 2.0);
  g.cy = (float)((ny - 1) / 2.0);
  g.r2 = (float)(r * r);
  g.drho = (float)(n_rho > 1 ? 2.0 * std::floor(r) / (n_rho - 1) : 1.0);
  g.dtheta = (float)(3.141592653589793 / n_theta);
  for (int i = 0; i < ny; ++i)
    for (int j = 0; j < nx; ++j) g.n_mask += hough_in_mask(g, i, j) ? 1 : 0;
  return g;
}

HOUGH_HD float hough_rho(const HoughGeom &g, float k) { return (k - (float)(g.n_rho - 1) * 0.5f) * g.drho; }

// staged pixel (i, j), 0 outside the pattern
HOUGH_HD float hough_pixel(const float *p, const HoughGeom &g, int i, int j) {
  return (i >= 0 && i < g.ny && j >= 0 && j < g.nx) ? p[(size_t)i * g.nx + j] : 0.0f;
}

// S[a][k] of a staged pattern
HOUGH_HD float hough_line_sum(const float *p, const HoughGeom &g, float c, float s, int k) {
  const float rho = hough_rho(g, (float)k);
  const float x0 = g.cx + rho * c, y0 = g.cy + rho * s, rr = rho * rho;
  float acc = 0.0f;
  for (int t = -g.t_half; t <= g.t_half; ++t) {
    const float tf = (float)t;
    if (rr + tf * tf > g.r2) continue;
    const float x = x0 - tf * s, y = y0 + tf * c;
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int j = (int)xf, i = (int)yf;
    const float v00 = hough_pixel(p, g, i, j), v01 = hough_pixel(p, g, i, j + 1);
    const float v10 = hough_pixel(p, g, i + 1, j), v11 = hough_pixel(p, g, i + 1, j + 1);
    const float top = v00 + fx * (v01 - v00), bot = v10 + fx * (v11 - v10);
    acc += top + fy * (bot - top);
  }
  return acc;
}

// the cell theta-neighbour (a + d, k) of the periodic sinogram: a wraps with rho flipped
HOUGH_HD void hough_wrap(const HoughGeom &g, int a, int k, int *aw, int *kw) {
  *aw = a;
  *kw = k;
  if (a < 0) {
    *aw = a + g.n_theta;
    *kw = g.n_rho - 1 - k;
  } else if (a >= g.n_theta) {
    *aw = a - g.n_theta;
    *kw = g.n_rho - 1 - k;
  }
}

// smoothing along rho (zeros beyond the ends) and along theta (the seam), taps in ascending order
HOUGH_HD float hough_smooth_rho(const float *s, const HoughGeom &g, const HoughSmooth &w, int a, int k) {
  float acc = 0.0f;
  for (int d = -w.rr; d <= w.rr; ++d) {
    const int kk = k + d;
    if (kk >= 0 && kk < g.n_rho) acc += w.wr[d + w.rr] * s[(size_t)a * g.n_rho + kk];
  }
  return acc;
}

HOUGH_HD float hough_smooth_theta(const float *s, const HoughGeom &g, const HoughSmooth &w, int a, int k) {
  float acc = 0.0f;
  for (int d = -w.rt; d <= w.rt; ++d) {
    int aw, kw;
    hough_wrap(g, a + d, k, &aw, &kw);
    acc += w.wt[d + w.rt] * s[(size_t)aw * g.n_rho + kw];
  }
  return acc;
}

// whether cell (a, k) of the smoothed sinogram u is a positive local maximum of its window: larger than every other
// cell of the window, or equal to it with the lower index a n_rho + k (a plateau has one maximum, its first cell)
HOUGH_HD bool hough_is_peak(const float *u, const HoughGeom &g, const HoughSmooth &w, int a, int k) {
  if (k < w.rim || k >= g.n_rho - w.rim) return false;
  const float c = u[(size_t)a * g.n_rho + k];
  if (!(c > 0.0f)) return false;
  const int here = a * g.n_rho + k;
  for (int da = -HOUGH_WINDOW; da <= HOUGH_WINDOW; ++da)
    for (int dk = -HOUGH_WINDOW; dk <= HOUGH_WINDOW; ++dk) {
      if (da == 0 && dk == 0) continue;
      int aw, kw;
      hough_wrap(g, a + da, k, &aw, &kw);
      kw += (aw == a + da) ? dk : -dk;  // across the seam the rho axis runs the other way
      if (kw < 0 || kw >= g.n_rho) continue;
      const int there = aw * g.n_rho + kw;
      if (there == here) continue;  // (a window wider than the theta axis)
      const float v = u[there];
      if (!(c > v || (c == v && here < there))) return false;
    }
  return true;
}

// offset of the vertex of the parabola through (-1, l), (0, c), (1, r), within half a cell; 0 where it has no maximum
HOUGH_HD float hough_vertex(float l, float c, float r) {
  const float den = (l - 2.0f * c) + r;
  if (!(den < 0.0f)) return 0.0f;
  float d = 0.5f * (l - r) / den;
  d = d < -0.5f ? -0.5f : d;
  return d > 0.5f ? 0.5f : d;
}

// the band at the peak cell (a, k)
HOUGH_HD HoughBand hough_band_at(const float *u, const HoughGeom &g, int a, int k) {
  HoughBand b;
  int al, kl, ar, kr;
  hough_wrap(g, a - 1, k, &al, &kl);
  hough_wrap(g, a + 1, k, &ar, &kr);
  const float c = u[(size_t)a * g.n_rho + k];
  b.da = hough_vertex(u[(size_t)al * g.n_rho + kl], c, u[(size_t)ar * g.n_rho + kr]);
  b.dk = hough_vertex(u[(size_t)a * g.n_rho + k - 1], c, u[(size_t)a * g.n_rho + k + 1]);  // (rim >= 1: both exist)
  b.theta = ((float)a + b.da) * g.dtheta;
  b.rho = hough_rho(g, (float)k + b.dk);
  b.value = c;
  b.valid = 1;
  b.a = a;
  b.k = k;
  return b;
}

// `x` comes before `y` in the order the strongest bands are taken in: larger value first, then the lower cell index
HOUGH_HD bool hough_before(float vx, int ix, float vy, int iy) { return vx > vy || (vx == vy && ix < iy); }

// ---- the launch plan ----------------------------------------------------------------------------------------------------
struct HoughPlan {
  bool ok;
  bool lds;                 // the staged pattern lives in LDS; else in the workspace
  size_t lds_bytes;         // dynamic LDS of the Radon kernel
  size_t pattern_bytes;     // workspace of one pattern: three sinograms (raw, tmp, smoothed) and the staged pattern (no LDS)
  int64_t pass_patterns, n_passes, tail_patterns;
};

// `room`: bytes the workspace may take; `forced` > 0: patterns per pass (tests)
inline HoughPlan hough_plan(int ny, int nx, int n_theta, int n_rho, int64_t m, size_t room, int64_t forced) {
  HoughPlan p{};
  // (n_theta: a window or a smoothing radius crosses the seam once at the most)
  if (ny < 3 || nx < 3 || ny > HOUGH_MAX_DIM || nx > HOUGH_MAX_DIM || n_theta < 2 * HOUGH_WINDOW + 1 || n_theta > HOUGH_MAX_DIM || n_rho < 3 ||
      n_rho > HOUGH_MAX_DIM || m < 1)
    return p;
  const size_t staged = (size_t)ny * nx * sizeof(float), sino = (size_t)n_theta * n_rho * sizeof(float);
  p.lds = staged + HOUGH_LDS_SCRATCH <= HOUGH_LDS_BYTES;
  p.lds_bytes = HOUGH_LDS_SCRATCH + (p.lds ? staged : 0);
  p.pattern_bytes = 3 * sino + (p.lds ? 0 : staged);
  int64_t per = forced > 0 ? forced : (int64_t)(room / p.pattern_bytes);
  if (per < 1) return p;
  if (per > m) per = m;
  if (per > 2147483647LL) per = 2147483647LL;
  p.pass_patterns = per;
  p.n_passes = (m + per - 1) / per;
  p.tail_patterns = m - (p.n_passes - 1) * per;
  p.ok = true;
  return p;
}

// ---- the launch plan of the projection-centre search (hough.hip, hough_pc_search_kernel; hough_search.h) -------------------
// One lane per pattern, and a lane's evaluation costs the same however many of its wave are idle: while there are fewer
// patterns than a full wave per CU would take, a workgroup holds fewer lanes - the power of two that still covers
// ceil(m / n_cu) - so that a small grid spreads over the CUs instead of filling one wave of one CU; 64 once m is large.
// `forced` > 0: lanes per workgroup (tests).  The result of a search does not depend on the plan.
constexpr int HOUGH_SEARCH_MAX_LANES = 64;
// evaluations per lane and launch by default: a bound on a kernel's duration.  A launch of ONE evaluation per lane of a 10 x 10
// grid of 60 x 60 patterns was measured at 81 ms (profiles/hough_pc_search.json): 6 stay under half a second, 16 did not
constexpr int HOUGH_SEARCH_EVALS = 6;
// the most evaluations one search may be allowed (its maxfev, or 4 + 5 maxiter where maxfev is unlimited): 16 times SciPy's
// default budget of 600.  A larger budget is refused, so that no single call can hold a GPU for an unbounded time
constexpr int64_t HOUGH_SEARCH_MAX_EVALS = 10000;

struct HoughSearchPlan {
  bool ok;
  int lanes;           // per workgroup: 1, 2, 4, ... 64
  int64_t workgroups;  // ceil(m / lanes)
};

HOUGH_HD HoughSearchPlan hough_search_plan(int64_t m, int n_cu, int forced = 0) {
  HoughSearchPlan p{};
  if (m < 1 || n_cu < 1 || forced < 0 || forced > HOUGH_SEARCH_MAX_LANES) return p;
  int lanes = 1;
  if (forced > 0) {
    lanes = forced;
  } else {
    const int64_t per_cu = (m + n_cu - 1) / n_cu;
    while (lanes < HOUGH_SEARCH_MAX_LANES && lanes < per_cu) lanes *= 2;
  }
  p.lanes = lanes;
  p.workgroups = (m + lanes - 1) / lanes;
  p.ok = p.workgroups <= 2147483647LL;
  return p;
}

// what the launches take
struct HoughBandsLaunch {
  const void *patterns;  // [n][ny][nx] of `dtype`, device
  int dtype;
  int64_t n;
  HoughGeom geom;
  HoughSmooth smooth;
  HoughPlan plan;
  int n_bands;
  const float *cos_sin;  // [2][n_theta]: the cosines, then the sines
  float *workspace;      // n * plan.pattern_bytes
  HoughBand *bands;      // [n][n_bands]
};

}  // namespace kpdi
