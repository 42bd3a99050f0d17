// hough_ops.hip - host side of Hough indexing (include/kpdi.h, kpdi_hough_*): argument checks, the tables the kernels of
// hough.hip take (cos / sin, smoothing taps, a phase's reflectors), the passes over the sinogram workspace.
#include "context.h"

using namespace kpdi;

namespace {

int64_t forced_pass() {
  const char *e = getenv("KPDI_HOUGH_PASS");  // tests: patterns per pass
  return e && atoll(e) > 0 ? atoll(e) : 0;
}

// evaluations per lane and launch of the projection-centre search: the caller's number, else KPDI_HOUGH_SEARCH_EVALS, else
// HOUGH_SEARCH_EVALS (6).  A bound on how long one kernel runs, not a tuning knob.
int search_evals(int asked) {
  if (asked > 0) return asked;
  const char *e = getenv("KPDI_HOUGH_SEARCH_EVALS");
  return e && atoi(e) > 0 ? atoi(e) : HOUGH_SEARCH_EVALS;
}

}  // namespace

extern "C" {

int kpdi_hough_default_n_rho(int ny, int nx) { return ny < 3 || nx < 3 ? 0 : hough_default_n_rho(ny, nx); }

int kpdi_hough_plan_describe(int ny, int nx, int n_theta, int n_rho, int64_t m, int64_t room_bytes, int64_t forced, int64_t *desc) {
  if (!desc) return fail(KPDI_EINVAL, "desc is NULL");
  const HoughPlan p = hough_plan(ny, nx, n_theta, n_rho, m, room_bytes > 0 ? (size_t)room_bytes : 0, forced);
  const int64_t v[7] = {p.ok, p.lds, (int64_t)p.lds_bytes, (int64_t)p.pattern_bytes, p.pass_patterns, p.n_passes, p.tail_patterns};
  std::copy(v, v + 7, desc);
  return KPDI_OK;
}

int kpdi_hough_bands(kpdi_ctx *c, int n_theta, int n_rho, const float *cos_sin, const float *theta_taps, int theta_radius,
                     const float *rho_taps, int rho_radius, int rim, int n_bands, void *bands_out, float *sinogram_out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  const int d = c->exp_dtype;
  if (!(d == KPDI_U8 || d == KPDI_I8 || d == KPDI_U16 || d == KPDI_I16 || d == KPDI_F32 || d == KPDI_F64))
    return fail(KPDI_EINVAL, "Hough indexing takes uint8/int8/uint16/int16/float32/float64 patterns");
  if (!bands_out || !cos_sin || !theta_taps || !rho_taps) return fail(KPDI_EINVAL, "bands_out, cos_sin or a tap table is NULL");
  if (n_bands < 1 || n_bands > HOUGH_MAX_BANDS) return fail(KPDI_EINVAL, "%d bands: between 1 and %d", n_bands, HOUGH_MAX_BANDS);
  const int max_radius = (HOUGH_MAX_TAPS - 1) / 2;
  if (theta_radius < 0 || theta_radius > max_radius || rho_radius < 0 || rho_radius > max_radius || theta_radius > n_theta)
    return fail(KPDI_EINVAL, "smoothing radii %d and %d: between 0 and %d, the first within the %d theta cells", theta_radius,
                rho_radius, max_radius, n_theta);
  if (rim < 1 || 2 * rim >= n_rho) return fail(KPDI_EINVAL, "a rim of %d of %d rho cells: at least 1, and a cell must be left", rim, n_rho);
  const int sy = c->sy, sx = c->sx;
  int rc = use_device(c);
  if (rc) return rc;
  bool dummy = false;
  rc = flush_preprocess(c, false, &dummy);  // the recorded background steps run first
  if (rc) return rc;
  size_t free_bytes = 0, total_bytes = 0;
  HIPCHK(hipMemGetInfo(&free_bytes, &total_bytes));
  const size_t room = (free_bytes + c->hough_ws.cap) / 2;
  HoughBandsLaunch l{};
  l.plan = hough_plan(sy, sx, n_theta, n_rho, c->m_all, room, forced_pass());
  if (!l.plan.ok)
    return fail(l.plan.pattern_bytes ? KPDI_ENOMEM : KPDI_EINVAL, "Hough transform of %lld patterns of %d x %d into %d x %d cells: "
                "a detector of 3 ... %d pixels a side and 7 ... %d x 3 ... %d cells are taken, one pattern's workspace is %zu "
                "bytes, %zu are free", (long long)c->m_all, sy, sx, n_theta, n_rho, HOUGH_MAX_DIM, HOUGH_MAX_DIM, HOUGH_MAX_DIM,
                l.plan.pattern_bytes, free_bytes);
  l.geom = hough_geom(sy, sx, n_theta, n_rho);
  l.smooth.rt = theta_radius;
  l.smooth.rr = rho_radius;
  std::copy(theta_taps, theta_taps + 2 * theta_radius + 1, l.smooth.wt);
  std::copy(rho_taps, rho_taps + 2 * rho_radius + 1, l.smooth.wr);
  l.smooth.rim = rim;
  HIPCHK(c->hough_tab.reserve(2 * (size_t)n_theta * sizeof(float)));
  HIPCHK(hipMemcpyAsync(c->hough_tab.p, cos_sin, 2 * (size_t)n_theta * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // (the caller's table)
  HIPCHK(c->hough_ws.reserve((size_t)l.plan.pass_patterns * l.plan.pattern_bytes));
  HIPCHK(c->hough_bands.reserve((size_t)l.plan.pass_patterns * n_bands * sizeof(HoughBand)));
  l.dtype = d;
  l.n_bands = n_bands;
  l.cos_sin = c->hough_tab.as<float>();
  l.workspace = c->hough_ws.as<float>();
  l.bands = c->hough_bands.as<HoughBand>();
  const size_t cells = (size_t)n_theta * n_rho, es = dtype_size(d);
  for (int64_t pass = 0; pass < l.plan.n_passes; ++pass) {
    const int64_t first = pass * l.plan.pass_patterns;
    l.n = pass == l.plan.n_passes - 1 ? l.plan.tail_patterns : l.plan.pass_patterns;
    l.patterns = (const char *)c->exp_raw.p + (size_t)first * c->npix * es;
    hipError_t e = launch_hough_radon(l, c->stream);
    if (e == hipSuccess) e = launch_hough_bands(l, c->stream);
    if (e != hipSuccess) return fail(KPDI_EHIP, "Hough kernels: %s (%lld patterns of %d x %d)", hipGetErrorString(e), (long long)l.n, sy, sx);
    if (sinogram_out)
      HIPCHK(hipMemcpy2DAsync(sinogram_out + (size_t)first * cells, cells * sizeof(float), l.workspace, l.plan.pattern_bytes,
                              cells * sizeof(float), (size_t)l.n, hipMemcpyDeviceToHost, c->stream));
    rc = results_to_host(c, (char *)bands_out + (size_t)first * n_bands * sizeof(HoughBand), l.bands,
                         (size_t)l.n * n_bands * sizeof(HoughBand));
    if (rc) return rc;
  }
  return KPDI_OK;
}

int kpdi_hough_index(kpdi_ctx *c, const void *bands, int64_t m, int n_bands, const double *pcs, int64_t n_pc, int ny, int nx,
                     const double *s2d, const double *normals, const int32_t *family, int n_reflectors, int n_families,
                     const double *angles, double tol, double *quat, double *fit, double *cm, int32_t *nmatch) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!bands || !pcs || !s2d || !normals || !family || !angles || !quat || !fit || !cm || !nmatch)
    return fail(KPDI_EINVAL, "an array is NULL");
  if (m < 1 || (n_pc != 1 && n_pc != m)) return fail(KPDI_EINVAL, "%lld patterns with %lld projection centres: one, or one each", (long long)m, (long long)n_pc);
  if (n_bands < 1 || n_bands > HV_MAX_BANDS) return fail(KPDI_EINVAL, "%d bands: between 1 and %d", n_bands, HV_MAX_BANDS);
  if (n_reflectors < 1 || n_reflectors > HV_MAX_REFLECTORS || n_families < 1 || n_families > HV_MAX_FAMILIES)
    return fail(KPDI_EINVAL, "%d reflectors in %d families: at most %d in %d", n_reflectors, n_families, HV_MAX_REFLECTORS, HV_MAX_FAMILIES);
  for (int p = 0; p < n_reflectors; ++p)
    if (family[p] < 0 || family[p] >= n_families) return fail(KPDI_EINVAL, "reflector %d is of family %d of %d", p, family[p], n_families);
  if (ny < 2 || nx < 2 || !(tol > 0)) return fail(KPDI_EINVAL, "a detector of %d x %d pixels, a tolerance of %g rad", ny, nx, tol);
  int rc = use_device(c);
  if (rc) return rc;
  const size_t P = (size_t)n_reflectors, bn = 3 * P * 8, ba = P * P * 8, bf = P * 4;
  const size_t bb = (size_t)m * n_bands * sizeof(HoughBand), bp = (size_t)n_pc * 24, bo = (size_t)m * (6 * 8 + 4);
  HIPCHK(c->hough_tab.reserve(bn + ba + bf));
  HIPCHK(c->hough_bands.reserve(bb));
  HIPCHK(c->hough_pc.reserve(bp));
  HIPCHK(c->hough_out.reserve(bo));
  char *tab = (char *)c->hough_tab.p;
  HIPCHK(hipMemcpyAsync(tab, normals, bn, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(tab + bn, angles, ba, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(tab + bn + ba, family, bf, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->hough_bands.p, bands, bb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->hough_pc.p, pcs, bp, hipMemcpyHostToDevice, c->stream));
  HvPhase ph{n_reflectors, n_families, (const double *)tab, (const int32_t *)(tab + bn + ba), (const double *)(tab + bn), tol};
  HvDetector det{};
  det.ny = ny;
  det.nx = nx;
  std::copy(s2d, s2d + 9, det.s2d);
  double *o = c->hough_out.as<double>();
  hipError_t e = launch_hough_index(c->hough_bands.as<HoughBand>(), m, n_bands, c->hough_pc.as<double>(), n_pc, det, ph, o, o + 4 * m,
                                    o + 5 * m, (int32_t *)(o + 6 * m), c->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);  // the uploads read the caller's arrays
    return fail(KPDI_EHIP, "Hough index kernel: %s (%lld patterns)", hipGetErrorString(e), (long long)m);
  }
  rc = results_to_host(c, quat, o, (size_t)m * 32);
  if (rc == KPDI_OK) rc = results_to_host(c, fit, o + 4 * m, (size_t)m * 8);
  if (rc == KPDI_OK) rc = results_to_host(c, cm, o + 5 * m, (size_t)m * 8);
  if (rc == KPDI_OK) rc = results_to_host(c, nmatch, o + 6 * m, (size_t)m * 4);
  return rc;
}

int kpdi_hough_optimize_pc(kpdi_ctx *c, const void *bands, int64_t m, int n_bands, const double *pc0, int ny, int nx, const double *s2d,
                           const double *normals, const int32_t *family, int n_reflectors, int n_families, const double *angles,
                           double tol, double tol_deg, double xatol, double fatol, int maxiter, int maxfev, int evals_per_launch,
                           int lanes, double *pc, double *fun, int32_t *nfev, int32_t *nit, int32_t *status) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!bands || !pc0 || !s2d || !normals || !family || !angles || !pc || !fun || !nfev || !nit || !status)
    return fail(KPDI_EINVAL, "an array is NULL");
  if (m < 1 || m > 2147483647LL) return fail(KPDI_EINVAL, "%lld patterns: between 1 and 2^31 - 1", (long long)m);
  if (n_bands < 1 || n_bands > HV_MAX_BANDS) return fail(KPDI_EINVAL, "%d bands: between 1 and %d", n_bands, HV_MAX_BANDS);
  if (n_reflectors < 1 || n_reflectors > HV_MAX_REFLECTORS || n_families < 1 || n_families > HV_MAX_FAMILIES)
    return fail(KPDI_EINVAL, "%d reflectors in %d families: at most %d in %d", n_reflectors, n_families, HV_MAX_REFLECTORS, HV_MAX_FAMILIES);
  for (int p = 0; p < n_reflectors; ++p)
    if (family[p] < 0 || family[p] >= n_families) return fail(KPDI_EINVAL, "reflector %d is of family %d of %d", p, family[p], n_families);
  if (ny < 2 || nx < 2 || !(tol > 0) || !(tol_deg > 0))
    return fail(KPDI_EINVAL, "a detector of %d x %d pixels, a tolerance of %g rad (%g degrees)", ny, nx, tol, tol_deg);
  if (evals_per_launch < 0 || lanes < 0 || lanes > HOUGH_SEARCH_MAX_LANES)
    return fail(KPDI_EINVAL, "%d evaluations per launch, %d lanes per workgroup: 0 (the default) or more, at most %d lanes",
                evals_per_launch, lanes, HOUGH_SEARCH_MAX_LANES);
  int rc = use_device(c);
  if (rc) return rc;
  HoughPcSearchLaunch l{};
  resolve_budget(3, maxiter, maxfev, &l.options.maxiter, &l.options.maxfun);
  std::copy(pc0, pc0 + 3, l.options.pc0);
  l.options.xatol = xatol;
  l.options.fatol = fatol;
  l.options.tol_deg = tol_deg;
  const HoughSearchPlan plan = hough_search_plan(m, c->n_cu, lanes);
  if (!plan.ok) return fail(KPDI_EINVAL, "no launch plan for %lld searches", (long long)m);
  const size_t P = (size_t)n_reflectors, bn = 3 * P * 8, ba = P * P * 8, bf = P * 4;
  const size_t bb = (size_t)m * n_bands * sizeof(HoughBand), bo = (size_t)m * (4 * 8 + 3 * 4);
  HIPCHK(c->hough_tab.reserve(bn + ba + bf));
  HIPCHK(c->hough_bands.reserve(bb));
  HIPCHK(c->hough_out.reserve(bo));
  HIPCHK(c->hough_search.reserve((size_t)m * sizeof(HoughPcSearch)));
  HIPCHK(c->hough_done.reserve((size_t)m));
  char *tab = (char *)c->hough_tab.p;
  HIPCHK(hipMemcpyAsync(tab, normals, bn, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(tab + bn, angles, ba, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(tab + bn + ba, family, bf, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->hough_bands.p, bands, bb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->hough_search.p, 0, (size_t)m * sizeof(HoughPcSearch), c->stream));  // all zero: not begun
  HIPCHK(hipStreamSynchronize(c->stream));  // (the uploads read the caller's arrays)
  l.bands = c->hough_bands.as<HoughBand>();
  l.m = m;
  l.n_bands = n_bands;
  l.det.ny = ny;
  l.det.nx = nx;
  std::copy(s2d, s2d + 9, l.det.s2d);
  l.phase = HvPhase{n_reflectors, n_families, (const double *)tab, (const int32_t *)(tab + bn + ba), (const double *)(tab + bn), tol};
  l.evals = search_evals(evals_per_launch);
  l.states = c->hough_search.as<HoughPcSearch>();
  l.done = c->hough_done.as<uint8_t>();
  // every search ends within its budget of evaluations, and with an unlimited one (maxiter given, maxfev not) within
  // maxiter iterations of at most 5 evaluations (reflection, contraction, three shrunk vertices) after the first 4
  const int64_t most_evals = l.options.maxfun < INT_MAX ? (int64_t)l.options.maxfun : 4 + 5 * (int64_t)l.options.maxiter;
  if (most_evals > HOUGH_SEARCH_MAX_EVALS)
    return fail(KPDI_EINVAL, "a budget of up to %lld evaluations per search (maxiter %d, maxfev %d): at most %lld on the device",
                (long long)most_evals, maxiter, maxfev, (long long)HOUGH_SEARCH_MAX_EVALS);
  const int64_t most_launches = (most_evals + l.evals - 1) / l.evals + 1;
  std::vector<uint8_t> done((size_t)m);
  bool all = false;
  for (int64_t launch = 0; launch < most_launches && !all; ++launch) {
    hipError_t e = launch_hough_pc_search(l, plan, c->stream);
    if (e != hipSuccess) return fail(KPDI_EHIP, "Hough projection-centre search kernel: %s (%lld patterns)", hipGetErrorString(e), (long long)m);
    rc = results_to_host(c, done.data(), l.done, (size_t)m);
    if (rc) return rc;
    all = std::all_of(done.begin(), done.end(), [](uint8_t d) { return d != 0; });
  }
  if (!all) return fail(KPDI_EHIP, "Hough projection-centre search: not every search ended within its budget of %lld evaluations", (long long)most_evals);
  double *o = c->hough_out.as<double>();
  int32_t *oi = (int32_t *)(o + 4 * m);
  hipError_t e = launch_hough_pc_search_results(l.states, m, o, o + 3 * m, oi, oi + m, oi + 2 * m, c->stream);
  if (e != hipSuccess) return fail(KPDI_EHIP, "Hough projection-centre results kernel: %s", hipGetErrorString(e));
  rc = results_to_host(c, pc, o, (size_t)m * 24);
  if (rc == KPDI_OK) rc = results_to_host(c, fun, o + 3 * m, (size_t)m * 8);
  if (rc == KPDI_OK) rc = results_to_host(c, nfev, oi, (size_t)m * 4);
  if (rc == KPDI_OK) rc = results_to_host(c, nit, oi + m, (size_t)m * 4);
  if (rc == KPDI_OK) rc = results_to_host(c, status, oi + 2 * m, (size_t)m * 4);
  return rc;
}

}  // extern "C"
