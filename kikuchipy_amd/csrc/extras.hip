// extras.hip - the rows either side of the sweep: dictionary generation on the device (master
// pattern, detector, projection - project.hip), refinement (refine.hip), the orientation similarity map (osm.hip).
// (one of the host translation units api.hip was split into in round 5: context.h holds what they share)
#include "context.h"

using namespace kpdi;

namespace kpdi {

int project_to_device(kpdi_ctx *c, const double *rotations, int64_t n, int rescale, double out_min, double out_max,
                      int dtype_out, void *d_out, const VarPc *var, bool stay_async) {
  if (!c->have_master) return fail(KPDI_EINVAL, "kpdi_set_master_pattern has not been called");
  if (!var && !c->have_dc) return fail(KPDI_EINVAL, "kpdi_set_detector has not been called");
  if (!rotations) return fail(KPDI_EINVAL, "rotations pointer is NULL");
  if (n <= 0 || n >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "need between 1 and 2^31-1 rotations per call");
  if (rescale && !(out_max > out_min)) return fail(KPDI_EINVAL, "rescale needs out_max > out_min");
  HIPCHK(c->rot.reserve((size_t)n * 7 * sizeof(double)));
  const size_t rot_bytes = (size_t)n * 4 * sizeof(double);
  if (stay_async && !var) {
    kpdi_ctx::RotStage &st = c->rot_stage[c->rot_next];
    if (st.copied) HIPCHK(hipEventSynchronize(st.copied));  // (four pushes ago: long done)
    if (st.pin.reserve(rot_bytes) == hipSuccess) {
      c->rot_next = (c->rot_next + 1) % 4;
      HIPCHK(st.copied.ensure());
      memcpy(st.pin.p, rotations, rot_bytes);
      HIPCHK(hipMemcpyAsync(c->rot.p, st.pin.p, rot_bytes, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipEventRecord(st.copied, c->stream));
    } else {  // no page-locked memory to be had: the synchronous way
      (void)hipGetLastError();
      stay_async = false;
    }
  }
  if (!stay_async || var) HIPCHK(hipMemcpyAsync(c->rot.p, rotations, rot_bytes, hipMemcpyHostToDevice, c->stream));
  c->cnt.h2d_bytes += (double)n * 4 * sizeof(double);
  kpdi::ProjectLaunch p{};
  p.rotations = c->rot.as<double>();
  p.n = n;
  if (var) {
    double *d_pcs = c->rot.as<double>() + (size_t)n * 4;
    HIPCHK(hipMemcpyAsync(d_pcs, var->pcs, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    p.pcs = d_pcs;
    p.nrows = var->nrows;
    p.ncols = var->ncols;
    for (int i = 0; i < 9; ++i) p.om[i] = var->om[i];
    p.direction_cosines = nullptr;
    p.npix = var->nrows * var->ncols;
  } else {
    p.direction_cosines = c->dcos.as<double>();
    p.npix = (int)c->dc_npix;
  }
  p.master_packed = c->mp_packed.as<float>();
  p.npx = c->mp_npx;
  p.npy = c->mp_npy;
  p.rescale = rescale;
  p.out_min = out_min;
  p.out_max = out_max;
  p.dtype_out = dtype_out;
  p.out = d_out;
  {
    ScopedTimer t(c, &c->ev_proj);
    HIPCHK(kpdi::launch_project(p, c->stream));
  }
  // the rotations buffer may be a temporary of the caller's binding: it must have been read
  // before we return (pageable memory is staged synchronously, pinned memory is not)
  if (!stay_async || var) HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

}  // namespace kpdi

extern "C" {

int kpdi_set_master_pattern(kpdi_ctx *c, const void *upper, const void *lower, int dtype, int npx, int npy) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!upper) return fail(KPDI_EINVAL, "upper hemisphere pointer is NULL");
  if (npx < 2 || npy < 2) return fail(KPDI_EINVAL, "master pattern must be at least 2 x 2 pixels");
  if (dtype != KPDI_U8 && dtype != KPDI_U16 && dtype != KPDI_F32 && dtype != KPDI_F64)
    return fail(KPDI_EINVAL, "master pattern dtype must be uint8, uint16, float32 or float64");
  int rc = use_device(c);
  if (rc) return rc;
  const size_t n = (size_t)npx * npy;
  std::vector<float> up(n), lo;
  auto convert = [&](const void *src, std::vector<float> &dst) {
    switch (dtype) {
      case KPDI_U8: for (size_t i = 0; i < n; ++i) dst[i] = (float)((const uint8_t *)src)[i]; break;
      case KPDI_U16: for (size_t i = 0; i < n; ++i) dst[i] = (float)((const uint16_t *)src)[i]; break;
      case KPDI_F32: for (size_t i = 0; i < n; ++i) dst[i] = ((const float *)src)[i]; break;
      default: for (size_t i = 0; i < n; ++i) dst[i] = (float)((const double *)src)[i]; break;
    }
  };
  convert(upper, up);
  if (lower && lower != upper) {
    lo.resize(n);
    convert(lower, lo);
  }
  std::vector<float> packed(kpdi::packed_master_floats(npx, npy));
  kpdi::pack_master_pattern(up.data(), lo.empty() ? up.data() : lo.data(), npx, npy, packed.data());
  HIPCHK(c->mp_packed.reserve(packed.size() * sizeof(float)));
  HIPCHK(hipMemcpyAsync(c->mp_packed.p, packed.data(), packed.size() * sizeof(float), hipMemcpyHostToDevice,
                        c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->cnt.h2d_bytes += (double)(packed.size() * sizeof(float));
  c->mp_npx = npx;
  c->mp_npy = npy;
  c->have_master = true;
  return KPDI_OK;
}

int kpdi_set_direction_cosines(kpdi_ctx *c, const double *dc, int64_t npix) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!dc) return fail(KPDI_EINVAL, "direction cosines pointer is NULL");
  if (npix <= 0 || npix >= (int64_t)INT_MAX / 3) return fail(KPDI_EINVAL, "bad number of detector pixels");
  int rc = use_device(c);
  if (rc) return rc;
  const size_t bytes = (size_t)npix * 3 * sizeof(double);
  HIPCHK(c->dcos.reserve(bytes));
  HIPCHK(hipMemcpyAsync(c->dcos.p, dc, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->dc_npix = npix;
  c->have_dc = true;
  return KPDI_OK;
}

int kpdi_set_detector(kpdi_ctx *c, const double *gb, double pcz, int nrows, int ncols, const double *om) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!gb || !om) return fail(KPDI_EINVAL, "gnomonic bounds / orientation matrix pointer is NULL");
  if (nrows <= 0 || ncols <= 0) return fail(KPDI_EINVAL, "detector must have at least one pixel");
  // _get_direction_cosines_for_fixed_pc (signals/util/_master_pattern.py:175-203)
  const double x_scale = (gb[1] - gb[0]) / ncols;
  const double y_scale = (gb[3] - gb[2]) / nrows;
  const double x_half = x_scale / 2, y_half = y_scale / 2;
  std::vector<double> dc((size_t)nrows * ncols * 3);
  for (int r = 0; r < nrows; ++r) {
    const double gy = gb[3] + r * (-y_scale);  // np.arange(y_max, y_min, -y_scale)[r]
    for (int col = 0; col < ncols; ++col) {
      const double gx = gb[0] + col * x_scale;  // np.arange(x_min, x_max, x_scale)[col]
      const double v[3] = {(gx + x_half) * pcz, (gy - y_half) * pcz, pcz};
      double w[3];
      for (int a = 0; a < 3; ++a) w[a] = v[0] * om[3 * a] + v[1] * om[3 * a + 1] + v[2] * om[3 * a + 2];
      const double norm = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
      double *o = &dc[((size_t)r * ncols + col) * 3];
      o[0] = w[0] / norm;
      o[1] = w[1] / norm;
      o[2] = w[2] / norm;
    }
  }
  return kpdi_set_direction_cosines(c, dc.data(), (int64_t)nrows * ncols);
}

int kpdi_get_direction_cosines(kpdi_ctx *c, double *out) {
  if (!c || !out) return fail(KPDI_EINVAL, "NULL argument");
  if (!c->have_dc) return fail(KPDI_EINVAL, "no detector set");
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, c->dcos.p, (size_t)c->dc_npix * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_project_patterns(kpdi_ctx *c, const double *rotations, int64_t n, int rescale, double out_min,
                          double out_max, int dtype_out, void *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!out) return fail(KPDI_EINVAL, "output pointer is NULL");
  if (dtype_out != KPDI_F32 && dtype_out != KPDI_F64 && dtype_out != KPDI_U8 && dtype_out != KPDI_U16)
    return fail(KPDI_EINVAL, "dtype_out must be float32, float64, uint8 or uint16");
  int rc = use_device(c);
  if (rc) return rc;
  if (!c->have_dc) return fail(KPDI_EINVAL, "kpdi_set_detector has not been called");
  const size_t bytes = (size_t)n * c->dc_npix * kpdi::dtype_size(dtype_out);
  if (n > 0) HIPCHK(c->proj_out.reserve(bytes));
  rc = project_to_device(c, rotations, n, rescale, out_min, out_max, dtype_out, c->proj_out.p);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, c->proj_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_project_patterns_varying_pc(kpdi_ctx *c, const double *rotations, const double *pcs, int64_t n, int nrows,
                                     int ncols, const double *om, int rescale, double out_min, double out_max,
                                     int dtype_out, void *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!out || !pcs || !om) return fail(KPDI_EINVAL, "NULL argument");
  if (nrows <= 0 || ncols <= 0) return fail(KPDI_EINVAL, "detector must have at least one pixel");
  if (dtype_out != KPDI_F32 && dtype_out != KPDI_F64 && dtype_out != KPDI_U8 && dtype_out != KPDI_U16)
    return fail(KPDI_EINVAL, "dtype_out must be float32, float64, uint8 or uint16");
  int rc = use_device(c);
  if (rc) return rc;
  const size_t bytes = (size_t)n * nrows * ncols * kpdi::dtype_size(dtype_out);
  if (n > 0) HIPCHK(c->proj_out.reserve(bytes));
  const VarPc var{pcs, nrows, ncols, om};
  rc = project_to_device(c, rotations, n, rescale, out_min, out_max, dtype_out, c->proj_out.p, &var);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(out, c->proj_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

}  // extern "C"

// ---- refinement ---------------------------------------------------------------
namespace {
int refine_mode_sizes(int mode, int *nvar, int *nfixed) {
  switch (mode) {
    case KPDI_REFINE_ORI: *nvar = 3; *nfixed = 3; return KPDI_OK;
    case KPDI_REFINE_PC: *nvar = 3; *nfixed = 4; return KPDI_OK;
    case KPDI_REFINE_ORI_PC: *nvar = 6; *nfixed = 0; return KPDI_OK;
  }
  return fail(KPDI_EINVAL, "unknown refinement mode %d", mode);
}

int refine_fill_launch(kpdi_ctx *c, int mode, kpdi::RefineLaunch *a) {
  if (!c->have_ref) return fail(KPDI_EINVAL, "kpdi_refine_set_patterns has not been called");
  if (!c->have_master) return fail(KPDI_EINVAL, "kpdi_set_master_pattern has not been called");
  int rc = refine_mode_sizes(mode, &a->nvar, &a->nfixed);
  if (rc) return rc;
  a->mode = mode;
  a->nrows = c->ref_nrows;
  a->ncols = c->ref_ncols;
  a->k = c->ref_k;
  a->rowcol = c->ref_rowcol.as<unsigned>();
  for (int i = 0; i < 9; ++i) a->om[i] = c->ref_om[i];
  a->master_packed = c->mp_packed.as<float>();
  a->npx = c->mp_npx;
  a->npy = c->mp_npy;
  a->patterns = c->ref_pat.as<float>();
  a->sqnorm = c->ref_sqn.as<double>();
  return KPDI_OK;
}
}  // namespace

extern "C" {

int kpdi_refine_set_patterns(kpdi_ctx *c, const void *patterns, int dtype, int64_t n, int nrows, int ncols,
                             const uint8_t *signal_mask, int rescale, const double *om) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!patterns || !om) return fail(KPDI_EINVAL, "patterns / orientation matrix pointer is NULL");
  const size_t es = kpdi::dtype_size(dtype);
  if (es == 0) return fail(KPDI_EINVAL, "unknown dtype %d", dtype);
  if (n <= 0 || n >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "need between 1 and 2^31-1 patterns");
  if (nrows <= 0 || ncols <= 0 || nrows > 65535 || ncols > 65535)
    return fail(KPDI_EINVAL, "detector shape must be within 1..65535 pixels per side");
  int rc = use_device(c);
  if (rc) return rc;
  const int npix = nrows * ncols;
  std::vector<int> map;
  std::vector<unsigned> rowcol;
  for (int i = 0; i < npix; ++i)
    if (!signal_mask || !signal_mask[i]) {
      map.push_back(i);
      rowcol.push_back(((unsigned)(i / ncols) << 16) | (unsigned)(i % ncols));
    }
  const int k = (int)map.size();
  if (k < 2) return fail(KPDI_EINVAL, "the signal mask must leave at least two pixels");
  const size_t bytes = (size_t)n * npix * es;
  HIPCHK(c->ref_raw.reserve(bytes));
  HIPCHK(c->ref_map.reserve((size_t)k * sizeof(int)));
  HIPCHK(c->ref_rowcol.reserve((size_t)k * sizeof(unsigned)));
  HIPCHK(c->ref_pat.reserve((size_t)n * k * sizeof(float)));
  HIPCHK(c->ref_sqn.reserve((size_t)n * sizeof(double)));
  HIPCHK(hipMemcpyAsync(c->ref_raw.p, patterns, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ref_map.p, map.data(), (size_t)k * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ref_rowcol.p, rowcol.data(), (size_t)k * sizeof(unsigned), hipMemcpyHostToDevice,
                        c->stream));
  c->cnt.h2d_bytes += (double)bytes;
  HIPCHK(kpdi::launch_refine_prep(c->ref_raw.p, dtype, n, npix, signal_mask ? c->ref_map.as<int>() : nullptr, k,
                                  rescale, c->ref_pat.as<float>(), c->ref_sqn.as<double>(), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // `map`, `rowcol` and the caller's buffer have been consumed
  c->ref_nrows = nrows;
  c->ref_ncols = ncols;
  c->ref_k = k;
  c->ref_n = n;
  for (int i = 0; i < 9; ++i) c->ref_om[i] = om[i];
  c->have_ref = true;
  return KPDI_OK;
}

int kpdi_refine_get_prepared(kpdi_ctx *c, float *patterns_out, double *sqnorm_out) {
  if (!c || !patterns_out || !sqnorm_out) return fail(KPDI_EINVAL, "NULL argument");
  if (!c->have_ref) return fail(KPDI_EINVAL, "kpdi_refine_set_patterns has not been called");
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(patterns_out, c->ref_pat.p, (size_t)c->ref_n * c->ref_k * sizeof(float), hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipMemcpyAsync(sqnorm_out, c->ref_sqn.p, (size_t)c->ref_n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_refine_objective(kpdi_ctx *c, int mode, int64_t n_eval, const int32_t *pattern_index, const double *x,
                          const double *fixed, double *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!pattern_index || !x || !out) return fail(KPDI_EINVAL, "NULL argument");
  if (n_eval <= 0 || n_eval >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "need between 1 and 2^31-1 evaluations");
  int rc = use_device(c);
  if (rc) return rc;
  kpdi::RefineLaunch a{};
  rc = refine_fill_launch(c, mode, &a);
  if (rc) return rc;
  if (a.nfixed > 0 && !fixed) return fail(KPDI_EINVAL, "this mode needs the `fixed` array");
  for (int64_t e = 0; e < n_eval; ++e)
    if (pattern_index[e] < 0 || pattern_index[e] >= c->ref_n)
      return fail(KPDI_EINVAL, "pattern index %d out of range at evaluation %lld", pattern_index[e], (long long)e);
  const size_t nx = (size_t)n_eval * a.nvar, nf = (size_t)n_eval * a.nfixed;
  HIPCHK(c->ref_in.reserve((nx + nf + 1) * sizeof(double)));
  HIPCHK(c->ref_idx.reserve((size_t)n_eval * sizeof(int)));
  HIPCHK(c->ref_out.reserve((size_t)n_eval * sizeof(double)));
  double *d_x = c->ref_in.as<double>(), *d_f = d_x + nx;
  HIPCHK(hipMemcpyAsync(d_x, x, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (nf) HIPCHK(hipMemcpyAsync(d_f, fixed, nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ref_idx.p, pattern_index, (size_t)n_eval * sizeof(int), hipMemcpyHostToDevice, c->stream));
  a.n_jobs = n_eval;
  a.x0 = d_x;
  a.fixed = d_f;
  HIPCHK(kpdi::launch_refine_objective(a, c->ref_idx.as<int>(), c->ref_out.as<double>(), c->stream));
  return results_to_host(c, out, c->ref_out.p, (size_t)n_eval * sizeof(double));
}

}  // extern "C"

// SciPy's resolution of maxiter / maxfev (scipy/optimize/_optimize.py, _minimize_neldermead); declared in context.h
void kpdi::resolve_budget(int nvar, int maxiter, int maxfev, int *it, int *fev) {
  const bool no_it = maxiter <= 0, no_fev = maxfev <= 0;
  if (no_it && no_fev) {
    *it = nvar * 200;
    *fev = nvar * 200;
  } else if (no_it) {
    *it = INT_MAX;
    *fev = maxfev;
  } else if (no_fev) {
    *it = maxiter;
    *fev = INT_MAX;
  } else {
    *it = maxiter;
    *fev = maxfev;
  }
}

namespace {
int nelder_mead_check_bounds(const double *lower, const double *upper, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (lower[i] > upper[i])
      return fail(KPDI_EINVAL, "Nelder Mead - one of the lower bounds is greater than an upper bound.");
  return KPDI_OK;
}

int powell_check_bounds(const double *lower, const double *upper, size_t count) {
  for (size_t i = 0; i < count; ++i) {
    if (!std::isfinite(lower[i]) || !std::isfinite(upper[i]))
      return fail(KPDI_EINVAL, "Powell - bounds must be finite for every variable (one-sided bounds are not built)");
    if (lower[i] > upper[i]) return fail(KPDI_EINVAL, "Powell - one of the lower bounds is greater than an upper bound.");
  }
  return KPDI_OK;
}

// the LN_NELDERMEAD search takes infinite bounds and leaves lower > upper to its own front end (INVALID_ARGS)
int nlopt_check_bounds(const double *lower, const double *upper, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (std::isnan(lower[i]) || std::isnan(upper[i])) return fail(KPDI_EINVAL, "LN_NELDERMEAD - a bound is NaN");
  return KPDI_OK;
}

// what nothing on the device would end: a search without ftol_rel and maxeval stops only when its simplex has
// collapsed, and one from a non-finite point never does
int nlopt_check_search(const double *x0, size_t count, const double *xstep, int nvar, double ftol_rel, int maxeval) {
  if (std::isnan(ftol_rel)) return fail(KPDI_EINVAL, "LN_NELDERMEAD - ftol_rel is NaN");
  if (!(ftol_rel > 0.0) && maxeval <= 0)
    return fail(KPDI_EINVAL, "LN_NELDERMEAD - give ftol_rel > 0 or maxeval > 0: nothing else ends the search");
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(x0[i])) return fail(KPDI_EINVAL, "LN_NELDERMEAD - a starting point is not finite");
  if (xstep)
    for (int i = 0; i < nvar; ++i)
      if (!std::isfinite(xstep[i])) return fail(KPDI_EINVAL, "LN_NELDERMEAD - an initial step is not finite");
  return KPDI_OK;
}

// SciPy's own validation of the options the device solver takes (scipy/optimize/_differentialevolution.py:823-831)
// and what the LDS population holds
int de_check_options(const kpdi::DeOptions &de) {
  if (de.members < 5 || de.members > KPDI_DE_POP_MAX)
    return fail(KPDI_EINVAL, "differential evolution - the population must have 5..%d members, got %d", KPDI_DE_POP_MAX,
                de.members);
  if (de.maxiter < 0) return fail(KPDI_EINVAL, "differential evolution - maxiter must not be negative");
  if (std::isnan(de.tol) || std::isnan(de.atol) || std::isnan(de.recombination))
    return fail(KPDI_EINVAL, "differential evolution - tol, atol or recombination is NaN");
  const bool pair = !std::isnan(de.mutation_hi);
  if (!(de.mutation_lo >= 0.0 && de.mutation_lo < 2.0) || (pair && !(de.mutation_hi >= de.mutation_lo && de.mutation_hi < 2.0)))
    return fail(KPDI_EINVAL, "differential evolution - the mutation constant must lie in [0, 2), a pair in order");
  if (de.init != 0 && de.init != 1)
    return fail(KPDI_EINVAL, "differential evolution - init must be 0 (latinhypercube) or 1 (random)");
  if (de.updating != 0 && de.updating != 1)
    return fail(KPDI_EINVAL, "differential evolution - updating must be 0 (immediate) or 1 (deferred)");
  return KPDI_OK;
}

// SciPy's own validation of the options the device solver takes (scipy/optimize/_basinhopping.py:644-647) and what
// would not end or not run there: an interval of 0 divides by zero, `range` of a negative niter is empty (refused here
// rather than guessed), a NaN among the options
int bh_check_options(const kpdi::BhOptions &bh, double xatol, double fatol) {
  if (bh.niter < 0) return fail(KPDI_EINVAL, "basinhopping - niter must not be negative");
  if (bh.interval < 1) return fail(KPDI_EINVAL, "basinhopping - interval must be at least 1");
  if (std::isnan(bh.T) || std::isnan(bh.stepsize) || std::isnan(bh.target_accept_rate) || std::isnan(bh.stepwise_factor) ||
      std::isnan(xatol) || std::isnan(fatol))
    return fail(KPDI_EINVAL, "basinhopping - an option is NaN");
  if (!std::isfinite(bh.stepsize) || !std::isfinite(2.0 * bh.stepsize))
    return fail(KPDI_EINVAL, "basinhopping - stepsize must be finite, and twice it too");
  if (!(bh.target_accept_rate > 0.0 && bh.target_accept_rate < 1.0))
    return fail(KPDI_EINVAL, "basinhopping - target_accept_rate has to be in range (0, 1)");
  if (!(bh.stepwise_factor > 0.0 && bh.stepwise_factor < 1.0))
    return fail(KPDI_EINVAL, "basinhopping - stepwise_factor has to be in range (0, 1)");
  return KPDI_OK;
}

int de_check_bounds(const double *lower, const double *upper, size_t count) {
  for (size_t i = 0; i < count; ++i) {
    if (!std::isfinite(lower[i]) || !std::isfinite(upper[i]))
      return fail(KPDI_EINVAL, "differential evolution - bounds must be finite for every variable");
    if (lower[i] > upper[i])
      return fail(KPDI_EINVAL, "differential evolution - one of the lower bounds is greater than an upper bound.");
  }
  return KPDI_OK;
}

// what a solver plugs into refine_solve: everything else of a solve is the same for every solver
struct RefineSolver {
  int (*check_bounds)(const double *lower, const double *upper, size_t count);
  // a.maxiter / a.maxfun from the caller's maxiter / maxfev (<= 0 = unset)
  void (*budget)(int nvar, int maxiter, int maxfev, int *it, int *fev);
  hipError_t (*launch)(const kpdi::RefineLaunch &a, int64_t trace_job, double *d_trace, int trace_capacity, hipStream_t s);
};

// one solve of n_patterns * n_starts jobs.  ref_in holds x0 | fixed | lower | upper, ref_out the result rows and, behind
// them, the `trace_capacity` rows (x[0..nvar), f) of job `trace_job` when the caller gives a `trace`
int refine_solve(kpdi_ctx *c, const RefineSolver &solver, int mode, int64_t n_patterns, int n_starts, const double *x0,
                 const double *fixed, const double *lower, const double *upper, double xtol, double ftol, int maxiter,
                 int maxfev, double *results, int64_t trace_job, double *trace, int trace_capacity,
                 const kpdi::NloptStep *xstep = nullptr, const kpdi::DeOptions *de = nullptr,
                 const kpdi::BhOptions *bh = nullptr) {
  // de: differential evolution - no x0, `de->seeds` one seed per job on the HOST; bh: basinhopping - `bh->seeds` alike
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if ((!x0 && !de) || !results) return fail(KPDI_EINVAL, "NULL argument");
  if ((lower == nullptr) != (upper == nullptr)) return fail(KPDI_EINVAL, "give both bounds or neither");
  if (n_starts <= 0) return fail(KPDI_EINVAL, "need at least one start per pattern");
  int rc = use_device(c);
  if (rc) return rc;
  kpdi::RefineLaunch a{};
  rc = refine_fill_launch(c, mode, &a);
  if (rc) return rc;
  if (n_patterns != c->ref_n)
    return fail(KPDI_EINVAL, "%lld patterns were set but starts for %lld were given", (long long)c->ref_n,
                (long long)n_patterns);
  if (a.nfixed > 0 && !fixed) return fail(KPDI_EINVAL, "this mode needs the `fixed` array");
  const int64_t jobs = n_patterns * n_starts;
  if (jobs >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "too many (pattern, start) pairs");
  if (trace && (trace_capacity <= 0 || trace_job < 0 || trace_job >= jobs))
    return fail(KPDI_EINVAL, "the trace needs a capacity of at least 1 and a job within 0..%lld", (long long)jobs - 1);
  const size_t nx = (size_t)jobs * a.nvar, nf = (size_t)jobs * a.nfixed;
  if (lower && (rc = solver.check_bounds(lower, upper, nx))) return rc;
  if (de && !lower) return fail(KPDI_EINVAL, "differential evolution searches within bounds: give both");
  const size_t total = nx * (lower ? 3 : 1) + nf + 1;
  const size_t result_doubles = (size_t)jobs * kpdi::REFINE_RESULT_STRIDE;
  const size_t trace_doubles = trace ? (size_t)trace_capacity * (a.nvar + 1) : 0;
  HIPCHK(c->ref_in.reserve(total * sizeof(double)));
  HIPCHK(c->ref_out.reserve((result_doubles + trace_doubles) * sizeof(double)));
  double *d_x = c->ref_in.as<double>(), *d_f = d_x + nx, *d_lo = d_f + nf, *d_hi = d_lo + nx;
  double *d_trace = c->ref_out.as<double>() + result_doubles;
  if (x0) HIPCHK(hipMemcpyAsync(d_x, x0, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (nf) HIPCHK(hipMemcpyAsync(d_f, fixed, nf * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (lower) {
    HIPCHK(hipMemcpyAsync(d_lo, lower, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_hi, upper, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if (de || bh) {
    HIPCHK(c->ref_idx.reserve((size_t)jobs * sizeof(uint32_t)));
    HIPCHK(hipMemcpyAsync(c->ref_idx.p, de ? de->seeds : bh->seeds, (size_t)jobs * sizeof(uint32_t),
                          hipMemcpyHostToDevice, c->stream));
    if (de) {
      a.de = *de;
      a.de.seeds = c->ref_idx.as<uint32_t>();
    } else {
      a.bh = *bh;
      a.bh.seeds = c->ref_idx.as<uint32_t>();
    }
  }
  HIPCHK(hipMemsetAsync(c->ref_out.p, 0, (result_doubles + trace_doubles) * sizeof(double), c->stream));
  a.n_jobs = jobs;
  a.n_starts = n_starts;
  a.x0 = x0 ? d_x : nullptr;
  a.fixed = d_f;
  a.lower = lower ? d_lo : nullptr;
  a.upper = lower ? d_hi : nullptr;
  a.xatol = xtol;
  a.fatol = ftol;
  solver.budget(a.nvar, maxiter, maxfev, &a.maxiter, &a.maxfun);
  if (xstep) a.xstep = *xstep;
  a.results = c->ref_out.as<double>();
  kpdi::EventPair timer(c);
  HIPCHK(timer.begin());
  HIPCHK(solver.launch(a, trace_job, trace ? d_trace : nullptr, trace_capacity, c->stream));
  HIPCHK(timer.end());
  if (trace)
    HIPCHK(hipMemcpyAsync(trace, d_trace, trace_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  rc = results_to_host(c, results, c->ref_out.p, result_doubles * sizeof(double));
  if (rc) return rc;
  float ms = 0.f;
  HIPCHK(timer.elapsed(&ms));
  c->cnt.refine_ms += ms;
  return KPDI_OK;
}

// one job of an optimiser's self-test: x0 | lower | upper into ref_in (`lo` and `hi` stay NULL without bounds) and room
// for `n_out` doubles in ref_out
struct SelftestIn {
  double *x, *lo, *hi;
};

int selftest_upload(kpdi_ctx *c, int nvar, const double *x0, const double *lower, const double *upper, int n_out,
                    SelftestIn *in) {
  HIPCHK(c->ref_in.reserve((size_t)(3 * nvar + 1) * sizeof(double)));
  HIPCHK(c->ref_out.reserve((size_t)n_out * sizeof(double)));
  in->x = c->ref_in.as<double>();
  in->lo = lower ? in->x + nvar : nullptr;
  in->hi = lower ? in->x + 2 * nvar : nullptr;
  HIPCHK(hipMemcpyAsync(in->x, x0, nvar * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (lower) {
    HIPCHK(hipMemcpyAsync(in->lo, lower, nvar * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(in->hi, upper, nvar * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  return KPDI_OK;
}

int selftest_download(kpdi_ctx *c, double *result, int n_out) {
  HIPCHK(hipMemcpyAsync(result, c->ref_out.p, (size_t)n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}
}  // namespace

extern "C" {

int kpdi_refine_solve(kpdi_ctx *c, int mode, int64_t n_patterns, int n_starts, const double *x0, const double *fixed,
                      const double *lower, const double *upper, double xatol, double fatol, int maxiter, int maxfev,
                      double *results) {
  static const RefineSolver nelder_mead = {
      nelder_mead_check_bounds, resolve_budget,
      [](const kpdi::RefineLaunch &a, int64_t, double *, int, hipStream_t s) { return kpdi::launch_refine_solve(a, s); }};
  return refine_solve(c, nelder_mead, mode, n_patterns, n_starts, x0, fixed, lower, upper, xatol, fatol, maxiter, maxfev,
                      results, 0, nullptr, 0);
}

int kpdi_nelder_mead_selftest(kpdi_ctx *c, int kind, int nvar, const double *x0, const double *lower,
                              const double *upper, double xatol, double fatol, int maxiter, int maxfev,
                              double *result) {
  if (!c || !x0 || !result) return fail(KPDI_EINVAL, "NULL argument");
  if (kind < 0 || kind > 4) return fail(KPDI_EINVAL, "kind must be within 0..4");
  if (nvar < 1 || nvar > 6) return fail(KPDI_EINVAL, "nvar must be within 1..6");
  if ((lower == nullptr) != (upper == nullptr)) return fail(KPDI_EINVAL, "give both bounds or neither");
  int rc = use_device(c);
  if (rc) return rc;
  SelftestIn in;
  rc = selftest_upload(c, nvar, x0, lower, upper, 3 + nvar, &in);
  if (rc) return rc;
  int it, fev;
  resolve_budget(nvar, maxiter, maxfev, &it, &fev);
  HIPCHK(kpdi::launch_nelder_mead_selftest(kind, nvar, in.x, in.lo, in.hi, xatol, fatol, it, fev,
                                           c->ref_out.as<double>(), c->stream));
  return selftest_download(c, result, 3 + nvar);
}

int kpdi_refine_solve_powell(kpdi_ctx *c, int mode, int64_t n_patterns, int n_starts, const double *x0,
                             const double *fixed, const double *lower, const double *upper, double xtol, double ftol,
                             int maxiter, int maxfev, double *results, int64_t trace_job, double *trace,
                             int trace_capacity) {
  // the budget goes through as given: Powell's rule (N * 1000 each, or the other unlimited) resolves it in powell.h
  static const RefineSolver powell = {powell_check_bounds,
                                      [](int, int maxiter, int maxfev, int *it, int *fev) {
                                        *it = maxiter;
                                        *fev = maxfev;
                                      },
                                      kpdi::launch_refine_solve_powell};
  return refine_solve(c, powell, mode, n_patterns, n_starts, x0, fixed, lower, upper, xtol, ftol, maxiter, maxfev, results,
                      trace_job, trace, trace_capacity);
}

int kpdi_powell_selftest(kpdi_ctx *c, int kind, int nvar, const double *x0, const double *lower, const double *upper,
                         double xtol, double ftol, int maxiter, int maxfev, double *result) {
  if (!c || !x0 || !result) return fail(KPDI_EINVAL, "NULL argument");
  if (kind < 0 || kind > 4) return fail(KPDI_EINVAL, "kind must be within 0..4");
  if (nvar < 1 || nvar > 6) return fail(KPDI_EINVAL, "nvar must be within 1..6");
  if ((lower == nullptr) != (upper == nullptr)) return fail(KPDI_EINVAL, "give both bounds or neither");
  int rc;
  if (lower && (rc = powell_check_bounds(lower, upper, (size_t)nvar))) return rc;
  rc = use_device(c);
  if (rc) return rc;
  SelftestIn in;
  rc = selftest_upload(c, nvar, x0, lower, upper, 4 + nvar, &in);
  if (rc) return rc;
  HIPCHK(kpdi::launch_powell_selftest(kind, nvar, in.x, in.lo, in.hi, xtol, ftol, maxiter, maxfev,
                                      c->ref_out.as<double>(), c->stream));
  return selftest_download(c, result, 4 + nvar);
}

int kpdi_refine_solve_nlopt(kpdi_ctx *c, int mode, int64_t n_patterns, int n_starts, const double *x0,
                            const double *fixed, const double *lower, const double *upper, const double *xstep,
                            double ftol_rel, int maxeval, double *results) {
  static const RefineSolver nlopt = {
      nlopt_check_bounds,
      [](int, int, int maxeval, int *it, int *fev) {
        *it = 0;
        *fev = maxeval;
      },
      [](const kpdi::RefineLaunch &a, int64_t, double *, int, hipStream_t s) { return kpdi::launch_refine_solve_nlopt(a, s); }};
  if (!x0) return fail(KPDI_EINVAL, "NULL argument");
  int nvar, nfixed;
  int rc = refine_mode_sizes(mode, &nvar, &nfixed);
  if (rc) return rc;
  if (n_patterns < 0 || n_starts <= 0 || n_patterns * n_starts >= (int64_t)INT_MAX)
    return fail(KPDI_EINVAL, "need at least one start per pattern and fewer than 2^31 (pattern, start) pairs");
  rc = nlopt_check_search(x0, (size_t)(n_patterns * n_starts) * nvar, xstep, nvar, ftol_rel, maxeval);
  if (rc) return rc;
  kpdi::NloptStep step{};
  if (xstep) {
    step.given = 1;
    for (int i = 0; i < nvar; ++i) step.v[i] = xstep[i];
  }
  return refine_solve(c, nlopt, mode, n_patterns, n_starts, x0, fixed, lower, upper, 0.0, ftol_rel, 0, maxeval, results, 0,
                      nullptr, 0, &step);
}

int kpdi_refine_solve_de(kpdi_ctx *c, int mode, int64_t n_patterns, int n_starts, const double *fixed, const double *lower,
                         const double *upper, int members, int maxiter, double tol, double atol, double mutation_lo,
                         double mutation_hi, double recombination, int init, int updating, const uint32_t *seeds,
                         double *results, int64_t trace_job, double *trace, int trace_capacity) {
  static const RefineSolver de_solver = {de_check_bounds,
                                         [](int, int maxiter, int, int *it, int *fev) {
                                           *it = maxiter;
                                           *fev = 0;
                                         },
                                         kpdi::launch_refine_solve_de};
  if (!lower || !upper || !seeds) return fail(KPDI_EINVAL, "NULL argument (bounds and seeds are required)");
  const kpdi::DeOptions de{members, maxiter, init, updating, tol, atol, mutation_lo, mutation_hi, recombination, seeds};
  int rc = de_check_options(de);
  if (rc) return rc;
  return refine_solve(c, de_solver, mode, n_patterns, n_starts, nullptr, fixed, lower, upper, tol, atol, maxiter, 0, results,
                      trace_job, trace, trace_capacity, nullptr, &de);
}

int kpdi_de_selftest(kpdi_ctx *c, int kind, int nvar, const double *lower, const double *upper, int members, int maxiter,
                     double tol, double atol, double mutation_lo, double mutation_hi, double recombination, int init,
                     int updating, uint32_t seed, double *result) {
  if (!c || !lower || !upper || !result) return fail(KPDI_EINVAL, "NULL argument");
  if (kind < 0 || kind > 7) return fail(KPDI_EINVAL, "kind must be within 0..7");
  if (nvar < 1 || nvar > 6) return fail(KPDI_EINVAL, "nvar must be within 1..6");
  const kpdi::DeOptions de{members, maxiter, init, updating, tol, atol, mutation_lo, mutation_hi, recombination, nullptr};
  int rc = de_check_options(de);
  if (rc) return rc;
  if ((rc = de_check_bounds(lower, upper, (size_t)nvar))) return rc;
  rc = use_device(c);
  if (rc) return rc;
  SelftestIn in;
  rc = selftest_upload(c, nvar, lower, lower, upper, 4 + nvar, &in);  // the x0 slot is not used
  if (rc) return rc;
  HIPCHK(kpdi::launch_de_selftest(kind, nvar, in.lo, in.hi, de, seed, c->ref_out.as<double>(), c->stream));
  return selftest_download(c, result, 4 + nvar);
}

int kpdi_refine_solve_basinhopping(kpdi_ctx *c, int mode, int64_t n_patterns, int n_starts, const double *x0,
                                   const double *fixed, int niter, double T, double stepsize, int interval,
                                   int niter_success, double target_accept_rate, double stepwise_factor, double xatol,
                                   double fatol, int maxiter, int maxfev, const uint32_t *seeds, double *results,
                                   int64_t trace_job, double *trace, int trace_capacity) {
  // unbounded: check_bounds is never called
  static const RefineSolver basinhopping = {nelder_mead_check_bounds, resolve_budget,
                                            kpdi::launch_refine_solve_basinhopping};
  if (!x0 || !seeds) return fail(KPDI_EINVAL, "NULL argument (starts and seeds are required)");
  const kpdi::BhOptions bh{niter, interval, niter_success, T, stepsize, target_accept_rate, stepwise_factor, seeds};
  int rc = bh_check_options(bh, xatol, fatol);
  if (rc) return rc;
  return refine_solve(c, basinhopping, mode, n_patterns, n_starts, x0, fixed, nullptr, nullptr, xatol, fatol, maxiter,
                      maxfev, results, trace_job, trace, trace_capacity, nullptr, nullptr, &bh);
}

int kpdi_basinhopping_selftest(kpdi_ctx *c, int kind, int nvar, const double *x0, int niter, double T, double stepsize,
                               int interval, int niter_success, double target_accept_rate, double stepwise_factor,
                               double xatol, double fatol, int maxiter, int maxfev, uint32_t seed, double *result) {
  if (!c || !x0 || !result) return fail(KPDI_EINVAL, "NULL argument");
  if (kind < 0 || kind > 4) return fail(KPDI_EINVAL, "kind must be within 0..4");
  if (nvar < 1 || nvar > 6) return fail(KPDI_EINVAL, "nvar must be within 1..6");
  const kpdi::BhOptions bh{niter, interval, niter_success, T, stepsize, target_accept_rate, stepwise_factor, nullptr};
  int rc = bh_check_options(bh, xatol, fatol);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  SelftestIn in;
  rc = selftest_upload(c, nvar, x0, nullptr, nullptr, 5 + nvar, &in);
  if (rc) return rc;
  int it, fev;
  resolve_budget(nvar, maxiter, maxfev, &it, &fev);
  HIPCHK(kpdi::launch_basinhopping_selftest(kind, nvar, in.x, bh, xatol, fatol, it, fev, seed, c->ref_out.as<double>(),
                                            c->stream));
  return selftest_download(c, result, 5 + nvar);
}

int kpdi_mt19937_selftest(kpdi_ctx *c, uint32_t seed, const double *program, int n, uint64_t *out, int64_t out_words) {
  if (!c || !program || !out) return fail(KPDI_EINVAL, "NULL argument");
  if (n < 1 || n > (1 << 16)) return fail(KPDI_EINVAL, "between 1 and 65536 draws");
  int64_t words = 0;
  for (int r = 0; r < n; ++r) {
    const double op = program[3 * r], a = program[3 * r + 1], b = program[3 * r + 2];
    if (!(op == 0 || op == 1 || op == 2 || op == 3 || op == 4)) return fail(KPDI_EINVAL, "draw %d: unknown op", r);
    if (op == 1 && !(std::isfinite(a) && std::isfinite(b))) return fail(KPDI_EINVAL, "draw %d: uniform(a, b) needs finite a, b", r);
    if (op >= 2 && !(a == std::floor(a) && a >= 1 && a < 2147483648.0)) return fail(KPDI_EINVAL, "draw %d: needs an integer a >= 1", r);
    if (op >= 3 && a > KPDI_DE_POP_MAX) return fail(KPDI_EINVAL, "draw %d: at most %d entries", r, KPDI_DE_POP_MAX);
    words += op >= 3 ? (int64_t)a : 1;
  }
  if (words != out_words) return fail(KPDI_EINVAL, "the program makes %lld words, room for %lld was given", (long long)words, (long long)out_words);
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(c->ref_in.reserve((size_t)3 * n * sizeof(double)));
  HIPCHK(c->ref_out.reserve((size_t)(words + 1) * sizeof(uint64_t)));
  HIPCHK(hipMemcpyAsync(c->ref_in.p, program, (size_t)3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(c->ref_out.p, 0, (size_t)(words + 1) * sizeof(uint64_t), c->stream));
  HIPCHK(kpdi::launch_mt19937_selftest(seed, c->ref_in.as<double>(), n, c->ref_out.as<uint64_t>(), words, c->stream));
  HIPCHK(hipMemcpyAsync(out, c->ref_out.p, (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_nlopt_simplex_selftest(kpdi_ctx *c, int kind, int nvar, const double *x0, const double *lower,
                                const double *upper, const double *xstep, double ftol_rel, int maxeval, double *result) {
  if (!c || !x0 || !result) return fail(KPDI_EINVAL, "NULL argument");
  if (kind < 0 || kind > 5) return fail(KPDI_EINVAL, "kind must be within 0..5");
  if (nvar < 1 || nvar > 6) return fail(KPDI_EINVAL, "nvar must be within 1..6");
  if ((lower == nullptr) != (upper == nullptr)) return fail(KPDI_EINVAL, "give both bounds or neither");
  int rc;
  if (lower && (rc = nlopt_check_bounds(lower, upper, (size_t)nvar))) return rc;
  if ((rc = nlopt_check_search(x0, (size_t)nvar, xstep, nvar, ftol_rel, maxeval))) return rc;
  rc = use_device(c);
  if (rc) return rc;
  // x0 | lower | upper | xstep
  SelftestIn in;
  HIPCHK(c->ref_in.reserve((size_t)(4 * nvar + 1) * sizeof(double)));
  rc = selftest_upload(c, nvar, x0, lower, upper, 3 + nvar, &in);
  if (rc) return rc;
  double *d_step = nullptr;
  if (xstep) {
    d_step = c->ref_in.as<double>() + 3 * nvar;
    HIPCHK(hipMemcpyAsync(d_step, xstep, nvar * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(kpdi::launch_nlopt_simplex_selftest(kind, nvar, in.x, in.lo, in.hi, d_step, ftol_rel, maxeval,
                                             c->ref_out.as<double>(), c->stream));
  return selftest_download(c, result, 3 + nvar);
}

// ---- the merge and fill kernels on caller-made lists (tests/test_gpu_merge.py) ------------------------------------
// Host arrays in, the whole output buffer out: a test decides every byte the kernels see, what lies behind a list's
// count included.  Every extent is checked against the buffer sizes given before anything is launched.
namespace {
struct Upload {
  DevBuf d;
  hipError_t put(const void *host, size_t bytes, hipStream_t s) {
    hipError_t e = d.reserve(bytes ? bytes : 4);
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpyAsync(d.p, host, bytes, hipMemcpyHostToDevice, s);
  }
};
}  // namespace

int kpdi_merge_selftest(kpdi_ctx *c, int n_src, const float *const *src_scores, const int32_t *const *src_idx,
                        const int32_t *const *src_cnt, const int64_t *src_elems, const int32_t *src_lists,
                        const int32_t *src_len, const int32_t *src_row_stride, const int32_t *src_list_stride, int m,
                        int k, int out_stride, int out_offset, int seg_n, const int32_t *seg_row0,
                        const int32_t *seg_delta, uint32_t seg_sources, float *out_scores, int32_t *out_idx, int force,
                        int32_t *launch_error, int32_t *plan_ran) {
  if (!c || !src_scores || !src_idx || !src_cnt || !src_elems || !src_lists || !src_len || !src_row_stride ||
      !src_list_stride || !out_scores || !out_idx || !launch_error || !plan_ran)
    return fail(KPDI_EINVAL, "NULL argument");
  if (n_src < 1 || n_src > 3) return fail(KPDI_EINVAL, "between 1 and 3 sources");
  if (m < 1 || k < 1 || out_offset < 0 || (int64_t)out_offset + k > out_stride)
    return fail(KPDI_EINVAL, "need m, k >= 1 and out_offset + k <= out_stride");
  if (seg_n < 0 || seg_n > kpdi::INDEX_SEGMENTS || (seg_n > 0 && (!seg_row0 || !seg_delta)))
    return fail(KPDI_EINVAL, "between 0 and %d segments", kpdi::INDEX_SEGMENTS);
  int64_t candidates = 0;
  for (int j = 0; j < n_src; ++j) {
    if (!src_scores[j] || !src_idx[j]) return fail(KPDI_EINVAL, "source %d: NULL lists", j);
    if (src_lists[j] < 1 || src_len[j] < 1 || src_row_stride[j] < 0 || src_list_stride[j] < 0)
      return fail(KPDI_EINVAL, "source %d: bad shape", j);
    const int64_t last = (int64_t)(m - 1) * src_row_stride[j] + (int64_t)(src_lists[j] - 1) * src_list_stride[j] + src_len[j];
    if (last > src_elems[j]) return fail(KPDI_EINVAL, "source %d: its lists end at element %lld of %lld", j, (long long)last, (long long)src_elems[j]);
    candidates += (int64_t)src_lists[j] * src_len[j];
  }
  if (candidates > (1 << 22)) return fail(KPDI_EINVAL, "too many candidates for a self-test");
  int rc = use_device(c);
  if (rc) return rc;
  Upload us[3], ui[3], uc[3], uos, uoi;
  kpdi::MergeLaunch l{};
  l.m = m;
  l.k = k;
  l.n_src = n_src;
  for (int j = 0; j < n_src; ++j) {
    HIPCHK(us[j].put(src_scores[j], (size_t)src_elems[j] * sizeof(float), c->stream));
    HIPCHK(ui[j].put(src_idx[j], (size_t)src_elems[j] * sizeof(int), c->stream));
    if (src_cnt[j]) HIPCHK(uc[j].put(src_cnt[j], (size_t)m * src_lists[j] * sizeof(int), c->stream));
    l.src_scores[j] = us[j].d.as<float>();
    l.src_idx[j] = ui[j].d.as<int>();
    l.src_cnt[j] = src_cnt[j] ? uc[j].d.as<int>() : nullptr;
    l.src_lists[j] = src_lists[j];
    l.src_len[j] = src_len[j];
    l.src_row_stride[j] = src_row_stride[j];
    l.src_list_stride[j] = src_list_stride[j];
  }
  const size_t n_out = (size_t)m * out_stride;
  HIPCHK(uos.put(out_scores, n_out * sizeof(float), c->stream));
  HIPCHK(uoi.put(out_idx, n_out * sizeof(int), c->stream));
  l.out_scores = uos.d.as<float>();
  l.out_idx = uoi.d.as<int>();
  l.out_stride = out_stride;
  l.out_offset = out_offset;
  l.seg.n = seg_n;
  for (int t = 0; t < kpdi::INDEX_SEGMENTS; ++t) {
    l.seg.row0[t] = t < seg_n ? seg_row0[t] : INT_MAX;
    l.seg.delta[t] = t < seg_n ? seg_delta[t] : 0;
  }
  l.seg_sources = seg_sources;
  int ran = -1;
  const hipError_t e = kpdi::launch_merge(l, c->stream, force, &ran);
  *launch_error = (int32_t)e;
  *plan_ran = ran;
  HIPCHK(hipMemcpyAsync(out_scores, uos.d.p, n_out * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(out_idx, uoi.d.p, n_out * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_merge64_selftest(kpdi_ctx *c, int m, int k, const double *run_s, const int32_t *run_i, int in_place,
                          const double *cand_s64, const int32_t *cand_i, int64_t cand_elems, int lists, int len,
                          int64_t row_stride, int64_t list_stride, const float *cand_s32, int s32_stride, int s32_col,
                          int enumerated_all, float max_diff, float eps_floor, double *out_s, int32_t *out_i,
                          int32_t *uncertified, int32_t *launch_error) {
  if (!c || !cand_s64 || !cand_i || !out_s || !out_i || !launch_error) return fail(KPDI_EINVAL, "NULL argument");
  if ((run_s == nullptr) != (run_i == nullptr)) return fail(KPDI_EINVAL, "give both halves of the running list or neither");
  if (in_place && !run_s) return fail(KPDI_EINVAL, "in place needs a running list");
  if ((cand_s32 == nullptr) != (uncertified == nullptr)) return fail(KPDI_EINVAL, "certification needs cand_s32 and uncertified");
  if (m < 1 || k < 1 || lists < 1 || len < 1 || row_stride < 0 || list_stride < 0) return fail(KPDI_EINVAL, "bad shape");
  if ((int64_t)(m - 1) * row_stride + (int64_t)(lists - 1) * list_stride + len > cand_elems)
    return fail(KPDI_EINVAL, "the candidate lists end behind their buffer");
  if (cand_s32 && (s32_col < 0 || s32_col >= s32_stride)) return fail(KPDI_EINVAL, "s32_col outside a row");
  int rc = use_device(c);
  if (rc) return rc;
  Upload urs, uri, ucs, uci, us32, uos, uoi, ucert;
  const size_t n_out = (size_t)m * k;
  if (run_s) {
    HIPCHK(urs.put(run_s, n_out * sizeof(double), c->stream));
    HIPCHK(uri.put(run_i, n_out * sizeof(int), c->stream));
  }
  HIPCHK(ucs.put(cand_s64, (size_t)cand_elems * sizeof(double), c->stream));
  HIPCHK(uci.put(cand_i, (size_t)cand_elems * sizeof(int), c->stream));
  HIPCHK(uos.put(out_s, n_out * sizeof(double), c->stream));
  HIPCHK(uoi.put(out_i, n_out * sizeof(int), c->stream));
  const unsigned cert[2] = {0u, 0u};  // (max_diff's bits, the counter)
  HIPCHK(ucert.put(cert, sizeof(cert), c->stream));
  HIPCHK(hipMemcpyAsync(ucert.d.p, &max_diff, sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (cand_s32) HIPCHK(us32.put(cand_s32, (size_t)m * s32_stride * sizeof(float), c->stream));
  kpdi::Merge64Launch g{};
  g.m = m;
  g.k = k;
  g.run_s = run_s ? urs.d.as<double>() : nullptr;
  g.run_i = run_s ? uri.d.as<int>() : nullptr;
  g.cand_s64 = ucs.d.as<double>();
  g.cand_i = uci.d.as<int>();
  g.lists = lists;
  g.len = len;
  g.row_stride = row_stride;
  g.list_stride = list_stride;
  g.out_s = in_place ? urs.d.as<double>() : uos.d.as<double>();
  g.out_i = in_place ? uri.d.as<int>() : uoi.d.as<int>();
  g.cand_s32 = cand_s32 ? us32.d.as<float>() : nullptr;
  g.s32_stride = s32_stride;
  g.s32_col = s32_col;
  g.enumerated_all = enumerated_all;
  g.max_diff = ucert.d.as<unsigned>();
  g.eps_floor = eps_floor;
  g.uncertified = cand_s32 ? (int *)(ucert.d.as<unsigned>() + 1) : nullptr;
  *launch_error = (int32_t)kpdi::launch_merge64(g, c->stream);
  HIPCHK(hipMemcpyAsync(out_s, g.out_s, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(out_i, g.out_i, n_out * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (uncertified) HIPCHK(hipMemcpyAsync(uncertified, ucert.d.as<unsigned>() + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

// rescore_kernel on caller-made patterns, maps and candidate lists (tests/test_gpu_rescore.py): every field of
// RescoreLaunch is the caller's; every index the kernel can form from them is checked here, so no launch reads or writes
// outside the uploaded buffers (a candidate index outside the chunk is the kernel's own business: it scores -inf).
int kpdi_rescore_selftest(kpdi_ctx *c, const void *exp_raw, int exp_dtype, int64_t m_all, const int32_t *row_map, int m,
                          const void *dict_raw, int dict_dtype, int64_t n_chunk, int64_t global_start,
                          const int32_t *pix_map, int k, int npix, int metric, const float *cand_s, const int32_t *cand_i,
                          int cand_stride, int cand_offset, int n_cand, float max_diff_in, double *cand_s64,
                          float *max_diff_out, int32_t *launch_error) {
  if (!c || !exp_raw || !dict_raw || !cand_s || !cand_i || !cand_s64 || !max_diff_out || !launch_error)
    return fail(KPDI_EINVAL, "NULL argument");
  if (exp_dtype < KPDI_U8 || exp_dtype > KPDI_F16 || dict_dtype < KPDI_U8 || dict_dtype > KPDI_F16)
    return fail(KPDI_EINVAL, "dtype codes %d / %d: not among the nine of kpdi.h", exp_dtype, dict_dtype);
  if (metric != KPDI_METRIC_NCC && metric != KPDI_METRIC_NDP) return fail(KPDI_EINVAL, "unknown metric %d", metric);
  if (k < 1) return fail(KPDI_EINVAL, "k must be at least 1");
  if (npix < 1 || m < 1 || m_all < 1 || n_chunk < 1 || global_start < 0 || global_start + n_chunk > (int64_t)INT_MAX)
    return fail(KPDI_EINVAL, "bad shape");
  if (m_all * npix > (1 << 24) || n_chunk * npix > (1 << 24) || (int64_t)m * cand_stride > (1 << 24) || k > (1 << 24))
    return fail(KPDI_EINVAL, "too large for a self-test");
  if (!pix_map && k > npix) return fail(KPDI_EINVAL, "k = %d kept pixels of %d need a pix_map", k, npix);
  if (!row_map && m > m_all) return fail(KPDI_EINVAL, "m = %d rows of %lld need a row_map", m, (long long)m_all);
  if (cand_offset < 0 || n_cand < 1 || (int64_t)cand_offset + n_cand > cand_stride)
    return fail(KPDI_EINVAL, "need cand_offset >= 0, n_cand >= 1 and cand_offset + n_cand <= cand_stride");
  if (!(max_diff_in >= 0.f)) return fail(KPDI_EINVAL, "max_diff is kept as the bits of a non-negative float");
  if (row_map)
    for (int r = 0; r < m; ++r)
      if (row_map[r] < 0 || row_map[r] >= m_all)
        return fail(KPDI_EINVAL, "row_map[%d] = %d is outside [0, %lld)", r, row_map[r], (long long)m_all);
  if (pix_map)
    for (int i = 0; i < k; ++i)
      if (pix_map[i] < 0 || pix_map[i] >= npix)
        return fail(KPDI_EINVAL, "pix_map[%d] = %d is outside [0, %d)", i, pix_map[i], npix);
  int rc = use_device(c);
  if (rc) return rc;
  Upload ue, ud, ur, up, us, ui, uo, um;
  const size_t n_cand_all = (size_t)m * cand_stride;
  HIPCHK(ue.put(exp_raw, (size_t)m_all * npix * kpdi_dtype_size(exp_dtype), c->stream));
  HIPCHK(ud.put(dict_raw, (size_t)n_chunk * npix * kpdi_dtype_size(dict_dtype), c->stream));
  if (row_map) HIPCHK(ur.put(row_map, (size_t)m * sizeof(int), c->stream));
  if (pix_map) HIPCHK(up.put(pix_map, (size_t)k * sizeof(int), c->stream));
  HIPCHK(us.put(cand_s, n_cand_all * sizeof(float), c->stream));
  HIPCHK(ui.put(cand_i, n_cand_all * sizeof(int), c->stream));
  HIPCHK(uo.put(cand_s64, n_cand_all * sizeof(double), c->stream));
  HIPCHK(um.put(&max_diff_in, sizeof(float), c->stream));
  kpdi::RescoreLaunch r{};
  r.exp_raw = ue.d.p;
  r.exp_dtype = exp_dtype;
  r.row_map = row_map ? ur.d.as<int>() : nullptr;
  r.dict_raw = ud.d.p;
  r.dict_dtype = dict_dtype;
  r.n_chunk = n_chunk;
  r.global_start = global_start;
  r.pix_map = pix_map ? up.d.as<int>() : nullptr;
  r.k = k;
  r.npix = npix;
  r.metric = metric;
  r.m = m;
  r.cand_s = us.d.as<float>();
  r.cand_i = ui.d.as<int>();
  r.cand_stride = cand_stride;
  r.cand_offset = cand_offset;
  r.n_cand = n_cand;
  r.cand_s64 = uo.d.as<double>();
  r.max_diff = um.d.as<unsigned>();
  *launch_error = (int32_t)kpdi::launch_rescore(r, c->stream);
  HIPCHK(hipMemcpyAsync(cand_s64, uo.d.p, n_cand_all * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(max_diff_out, um.d.p, sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_fill_selftest(kpdi_ctx *c, int n, const int64_t *words, const uint32_t *value, const int32_t *bound_used,
                       const int64_t *byte_offset, uint32_t *buffer, int64_t buffer_words) {
  if (!c || !words || !value || !bound_used || !byte_offset || !buffer) return fail(KPDI_EINVAL, "NULL argument");
  if (n < 0 || n > kpdi::FILL_SEGMENTS) return fail(KPDI_EINVAL, "between 0 and %d ranges", kpdi::FILL_SEGMENTS);
  if (buffer_words < 1 || buffer_words > (1 << 24)) return fail(KPDI_EINVAL, "bad buffer size");
  for (int i = 0; i < n; ++i)
    if (words[i] < 0 || byte_offset[i] < 0 || (byte_offset[i] & 3) || byte_offset[i] / 4 + words[i] > buffer_words ||
        bound_used[i] > kpdi::BOUND_SLOTS)
      return fail(KPDI_EINVAL, "range %d: outside the buffer, off a word boundary or bound_used > %d", i, kpdi::BOUND_SLOTS);
  int rc = use_device(c);
  if (rc) return rc;
  Upload u;
  HIPCHK(u.put(buffer, (size_t)buffer_words * 4, c->stream));
  kpdi::FillSegments f{};
  f.n = n;
  for (int i = 0; i < n; ++i) {
    f.p[i] = (unsigned *)((char *)u.d.p + byte_offset[i]);
    f.words[i] = (unsigned long long)words[i];
    f.value[i] = value[i];
    f.bound_used[i] = bound_used[i];
  }
  HIPCHK(kpdi::launch_fill_segments(f, c->stream));
  HIPCHK(hipMemcpyAsync(buffer, u.d.p, (size_t)buffer_words * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

// ---- orientation similarity map ---------------------------------------------------
int kpdi_orientation_similarity_map(kpdi_ctx *c, const int64_t *simulation_indices, int ny, int nx, int keep_n,
                                    int n_best, int from_n_best, const int32_t *footprint_offsets, int n_fp,
                                    int center_index, int normalize, float *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!footprint_offsets || !out) return fail(KPDI_EINVAL, "NULL argument");
  if (ny <= 0 || nx <= 0 || (int64_t)ny * nx >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "bad map shape");
  if (keep_n <= 0) return fail(KPDI_EINVAL, "keep_n must be positive");
  if (n_best > keep_n) return fail(KPDI_EINVAL, "n_best %d cannot be greater than keep_n %d", n_best, keep_n);
  if (from_n_best < 1 || from_n_best > n_best) return fail(KPDI_EINVAL, "from_n_best must be within 1..n_best");
  if (n_fp < 1 || n_fp > 64) return fail(KPDI_EINVAL, "the footprint must have between 1 and 64 points");
  if (center_index < 0 || center_index >= n_fp) return fail(KPDI_EINVAL, "center_index outside the footprint");
  int rc = use_device(c);
  if (rc) return rc;
  const size_t n_points = (size_t)ny * nx, n = n_points * keep_n;
  const int *d_idx = nullptr;
  if (simulation_indices) {
    std::vector<int> tmp(n);
    for (size_t i = 0; i < n; ++i) {
      if (simulation_indices[i] < INT_MIN || simulation_indices[i] > INT_MAX)
        return fail(KPDI_EINVAL, "simulation index %lld does not fit 32 bits", (long long)simulation_indices[i]);
      tmp[i] = (int)simulation_indices[i];
    }
    HIPCHK(c->osm_idx.reserve(n * sizeof(int)));
    HIPCHK(hipMemcpyAsync(c->osm_idx.p, tmp.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    d_idx = c->osm_idx.as<int>();
  } else {
    if (!c->final_valid) return fail(KPDI_EINVAL, "no resident result: call kpdi_finalize first");
    if ((size_t)c->m != n_points || c->keep_n != keep_n)
      return fail(KPDI_EINVAL, "the resident result is %d x %d but a %d x %d map with keep_n %d was asked for", c->m,
                  c->keep_n, ny, nx, keep_n);
    d_idx = c->final_idx;
  }
  const int n_layers = n_best - from_n_best + 1;
  HIPCHK(c->osm_out.reserve(n_points * n_layers * sizeof(float)));
  HIPCHK(kpdi::launch_osm(d_idx, ny, nx, keep_n, n_best, from_n_best, footprint_offsets, n_fp, center_index,
                          normalize != 0, c->osm_out.as<float>(), c->stream));
  return results_to_host(c, out, c->osm_out.p, n_points * n_layers * sizeof(float));
}

}  // extern "C"
