// pattern_ops.hip - host side of libkpdi.so, the ops on the resident experimental patterns: background removal,
// read-back, image quality, region sums, FFT filter, intensity rescaling / normalisation and range, adaptive histogram
// equalization, the neighbour ops, downsampling, the dynamic background, decomposition, dtype changes and selections - on
// top of the kernels in preproc.hip, iq.hip, regionsum.hip, fftfilter.hip, intensity.hip, clahe.hip, neighbours.hip,
// downsample.hip, decomp.hip, select.hip and reduce.hip (axis reductions).  Every op checks its arguments, then runs the
// recorded background steps (start_pattern_op).
#include "context.h"
#include "reduce_plan.h"

using namespace kpdi;

namespace kpdi {

// the six dtypes the ops on the resident patterns take; kpdi_set_experimental accepts dtypes 0 - 8, so this is "not
// float16 / int32 / uint32"
static bool intensity_dtype(int d) {
  return d == KPDI_U8 || d == KPDI_I8 || d == KPDI_U16 || d == KPDI_I16 || d == KPDI_F32 || d == KPDI_F64;
}

// what every op on the resident patterns checks first; `op` names it in the error text
static int check_patterns(kpdi_ctx *c, const char *op) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  if (!intensity_dtype(c->exp_dtype))
    return fail(KPDI_EINVAL, "%s takes uint8/int8/uint16/int16/float32/float64 patterns", op);
  return KPDI_OK;
}

// once its own arguments are checked: the device, then the recorded background-removal steps, which run first
static int start_pattern_op(kpdi_ctx *c) {
  int rc = use_device(c);
  if (rc) return rc;
  bool dummy = false;
  return flush_preprocess(c, false, &dummy);
}

// the resident patterns changed: what was prepared from them is stale
static void patterns_changed(kpdi_ctx *c) {
  c->exp_prepared = false;
  c->run_valid = false;
  discard_pending(c);
  c->final_valid = false;
}

// an op left its result in c->int_out: that becomes the resident set (in `dtype_out`, when the op chose one)
static void adopt_output(kpdi_ctx *c, int dtype_out = -1) {
  std::swap(c->exp_raw, c->int_out);
  if (dtype_out >= 0) c->exp_dtype = dtype_out;
  patterns_changed(c);
}

// a `dtype_out` that is none of the six: `what` = what the op does with them
static int bad_dtype_out(int dtype_out, const char *what) {
  return fail(KPDI_EINVAL, "dtype_out %d: %s uint8/int8/uint16/int16/float32/float64", dtype_out, what);
}

// (cos, sin)(2 pi j / n) as f32 pairs for j < sx, then for j < sy: 2 (sx + sy) floats
static void write_twiddles(float *tw, int sy, int sx) {
  for (int n : {sx, sy})
    for (int j = 0; j < n; ++j, tw += 2) {
      const double a = 2.0 * M_PI * j / n;
      tw[0] = (float)cos(a);
      tw[1] = (float)sin(a);
    }
}

// the normalised Gaussian window of the dynamic background in either domain, its length, centre and boundary mode
static int gaussian_taps(int filter_domain, double std, double truncate, std::vector<double> &taps, int *n_out,
                         int *centre_out, int *reflect_out) {
  int n;
  if (filter_domain == KPDI_DOMAIN_FREQUENCY) {
    // pattern/_pattern.py:604-613: n = int(truncate*std) samples of
    // scipy.signal.windows.gaussian, normalised; centre from filters/fft_barnes.py:106-117
    *n_out = n = (int)(truncate * std);
    if (n < 1) return fail(KPDI_EINVAL, "Gaussian window of int(truncate*std) = %d samples", n);
    taps.resize(n);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
      const double x = i - (n - 1) / 2.0;
      taps[i] = exp(-0.5 * (x / std) * (x / std));
      sum += taps[i];
    }
    for (double &t : taps) t /= sum;
    *centre_out = n - 1 - (n - 1) / 2;
    *reflect_out = 0;
  } else if (filter_domain == KPDI_DOMAIN_SPATIAL) {
    // scipy.ndimage.gaussian_filter(sigma=std, truncate=truncate), mode='reflect'
    const int r = (int)(truncate * std + 0.5);
    *n_out = n = 2 * r + 1;
    taps.resize(n);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
      const double x = i - r;
      taps[i] = exp(-0.5 / (std * std) * x * x);
      sum += taps[i];
    }
    for (double &t : taps) t /= sum;
    *centre_out = r;
    *reflect_out = 1;
  } else {
    return fail(KPDI_EINVAL, "unknown filter domain %d", filter_domain);
  }
  return KPDI_OK;
}

// the kernels read the taps through a window of CONV_R outputs: zero padding on both sides
static int upload_taps(kpdi_ctx *c, const std::vector<double> &taps) {
  std::vector<double> padded(taps.size() + 2 * (kpdi::CONV_R - 1), 0.0);
  std::copy(taps.begin(), taps.end(), padded.begin() + (kpdi::CONV_R - 1));
  HIPCHK(c->taps.reserve(padded.size() * sizeof(double)));
  HIPCHK(hipMemcpyAsync(c->taps.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // `padded` dies at scope exit
  return KPDI_OK;
}

}  // namespace kpdi

extern "C" {

int kpdi_remove_static_background(kpdi_ctx *c, const float *static_bg, int operation, int scale_bg) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  if (!static_bg) return fail(KPDI_EINVAL, "static_bg is NULL");
  if (c->exp_dtype == KPDI_F16 || c->exp_dtype == KPDI_I32 || c->exp_dtype == KPDI_U32)
    return fail(KPDI_EINVAL, "background removal takes uint8/int8/uint16/int16/float32/float64 patterns");
  if (operation != KPDI_OP_SUBTRACT && operation != KPDI_OP_DIVIDE) return fail(KPDI_EINVAL, "unknown operation");
  int rc = use_device(c);
  if (rc) return rc;
  // one static step followed by one dynamic step fuse into a single kernel; anything recorded that
  // this step cannot follow runs now
  bool dummy = false;
  if (c->pend.st || c->pend.dy) {
    rc = flush_preprocess(c, false, &dummy);
    if (rc) return rc;
  }
  HIPCHK(c->bg.reserve((size_t)c->npix * sizeof(float)));
  HIPCHK(hipMemcpyAsync(c->bg.p, static_bg, (size_t)c->npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // static_bg may be freed by the caller after return
  c->pend.st = true;
  c->pend.st_op = operation;
  c->pend.st_scale = scale_bg ? 1 : 0;
  c->pend.bg_min = *std::min_element(static_bg, static_bg + c->npix);
  c->pend.bg_max = *std::max_element(static_bg, static_bg + c->npix);
  patterns_changed(c);
  return KPDI_OK;
}

int kpdi_remove_dynamic_background(kpdi_ctx *c, int operation, int filter_domain, double std, double truncate) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  if (operation != KPDI_OP_SUBTRACT && operation != KPDI_OP_DIVIDE) return fail(KPDI_EINVAL, "unknown operation");
  if (c->exp_dtype == KPDI_F16 || c->exp_dtype == KPDI_I32 || c->exp_dtype == KPDI_U32)
    return fail(KPDI_EINVAL, "background removal takes uint8/int8/uint16/int16/float32/float64 patterns");
  int rc = use_device(c);
  if (rc) return rc;
  if (std <= 0) std = c->sx / 8.0;  // signals/ebsd.py:648-649
  std::vector<double> taps;
  int n, centre, reflect;
  rc = kpdi::gaussian_taps(filter_domain, std, truncate, taps, &n, &centre, &reflect);
  if (rc) return rc;
  bool dummy = false;
  if (c->pend.dy) {  // a second dynamic step cannot join the recorded one
    rc = flush_preprocess(c, false, &dummy);
    if (rc) return rc;
  }
  rc = kpdi::upload_taps(c, taps);
  if (rc) return rc;
  c->pend.dy = true;
  c->pend.dy_op = operation;
  c->pend.reflect = reflect;
  c->pend.ntaps = n;
  c->pend.centre = centre;
  patterns_changed(c);
  return KPDI_OK;
}

int kpdi_get_experimental(kpdi_ctx *c, void *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  int rc = kpdi::start_pattern_op(c);  // recorded background-removal steps run now
  if (rc) return rc;
  const size_t bytes = (size_t)c->m_all * c->npix * kpdi::dtype_size(c->exp_dtype);
  HIPCHK(hipMemcpyAsync(out, c->exp_raw.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_image_quality(kpdi_ctx *c, int normalize, const double *weights, double inertia_max, float *iq_out) {
  int rc = check_patterns(c, "image quality");
  if (rc) return rc;
  if (!iq_out) return fail(KPDI_EINVAL, "iq_out is NULL");
  const int sy = c->sy, sx = c->sx, h = kpdi::half_cols(sx);
  const kpdi::IqPlan plan = kpdi::image_quality_launch_plan(sy, sx, c->m_all);  // (what launch_image_quality follows)
  if (plan.path < 0) return fail(KPDI_EINVAL, "image quality of %d x %d patterns: no kernel path takes this shape", sy, sx);
  rc = start_pattern_op(c);
  if (rc) return rc;
  // weights w (pattern/_pattern.py:365-386 unless given), inertia_max = sum w / (sy sx) unless given
  std::vector<double> w((size_t)sy * sx);
  if (weights) {
    std::copy(weights, weights + w.size(), w.begin());
  } else {
    auto line = [](int n, int i) { return (long)(i < n / 2 ? i + 1 : i - n); };  // arange(n) + 1, [n//2:] -= n + 1
    for (int k = 0; k < sy; ++k)
      for (int l = 0; l < sx; ++l)
        w[(size_t)k * sx + l] = (double)(line(sy, k) * line(sy, k) + line(sx, l) * line(sx, l) - 1);
  }
  if (inertia_max <= 0) {
    double sum = 0;
    for (double v : w) sum += v;
    inertia_max = sum / ((double)sy * sx);
  }
  // folded weights of the half spectrum (iq.hip) and the twiddle tables: one upload
  const size_t wbytes = (size_t)sy * h * sizeof(double), tbytes = 2 * ((size_t)sx + sy) * sizeof(float);
  std::vector<char> tab(wbytes + tbytes);
  double *wf = (double *)tab.data();
  for (int k = 0; k < sy; ++k)
    for (int l = 0; l < h; ++l) {
      const bool self = l == 0 || 2 * l == sx;
      wf[(size_t)k * h + l] = w[(size_t)k * sx + l] + (self ? 0.0 : w[(size_t)((sy - k) % sy) * sx + (sx - l)]);
    }
  write_twiddles((float *)(tab.data() + wbytes), sy, sx);
  HIPCHK(c->op_tab.reserve(tab.size()));
  HIPCHK(hipMemcpyAsync(c->op_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c->iq_out.reserve((size_t)c->m_all * sizeof(float)));
  if (plan.path == 1) HIPCHK(c->op_ws.reserve(plan.workspace_bytes));
  kpdi::IqLaunch a;
  a.patterns = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.n = c->m_all;
  a.sy = sy;
  a.sx = sx;
  a.normalize = normalize ? 1 : 0;
  a.wfold = (const double *)c->op_tab.p;
  a.twiddles = (const float *)((const char *)c->op_tab.p + wbytes);
  a.inertia_max = inertia_max;
  a.workspace = c->op_ws.p;
  a.workspace_bytes = c->op_ws.cap;
  a.out = c->iq_out.as<float>();
  HIPCHK(kpdi::launch_image_quality(a, c->stream));
  return results_to_host(c, iq_out, c->iq_out.p, (size_t)c->m_all * sizeof(float));  // (synchronises: `tab` is read)
}

int kpdi_region_sums(kpdi_ctx *c, const int32_t *rects, int n_rects, void *sums_out) {
  int rc = check_patterns(c, "region sums");
  if (rc) return rc;
  if (n_rects < 0) return fail(KPDI_EINVAL, "n_rects is %d", n_rects);
  if (n_rects == 0) return KPDI_OK;
  if (!rects) return fail(KPDI_EINVAL, "rects is NULL");
  if (!sums_out) return fail(KPDI_EINVAL, "sums_out is NULL");
  const int sy = c->sy, sx = c->sx;
  for (int k = 0; k < n_rects; ++k) {
    const int32_t *r = rects + 4 * (size_t)k;
    if (r[0] < 0 || r[1] < r[0] || r[1] > sy || r[2] < 0 || r[3] < r[2] || r[3] > sx)
      return fail(KPDI_EINVAL, "rectangle %d, rows [%d, %d) and columns [%d, %d), is not inside the %d x %d detector", k,
                  r[0], r[1], r[2], r[3], sy, sx);
  }
  const kpdi::RsPlan plan = kpdi::rs_plan(c->exp_dtype, sy, sx, c->m_all, n_rects);
  if (plan.path < 0)
    return fail(KPDI_EINVAL, "region sums of %d x %d patterns over %d rectangles: no kernel path takes this shape", sy, sx,
                n_rects);
  rc = start_pattern_op(c);
  if (rc) return rc;
  const size_t rbytes = (size_t)n_rects * 4 * sizeof(int32_t);
  const size_t obytes = (size_t)c->m_all * n_rects * (c->exp_dtype == KPDI_F32 ? 4 : 8);
  HIPCHK(c->op_tab.reserve(rbytes));
  HIPCHK(hipMemcpyAsync(c->op_tab.p, rects, rbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c->iq_out.reserve(obytes));
  if (plan.path == 1) HIPCHK(c->op_ws.reserve(plan.workspace_bytes));
  kpdi::RsLaunch a{};
  a.patterns = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.n = c->m_all;
  a.sy = sy;
  a.sx = sx;
  a.rects = (const int32_t *)c->op_tab.p;
  a.n_rects = n_rects;
  a.workspace = c->op_ws.p;
  a.workspace_bytes = c->op_ws.cap;
  a.out = c->iq_out.p;
  hipError_t e = kpdi::launch_region_sums(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "region-sum kernel: %s (dtype %d, %dx%d, %d rectangles)", hipGetErrorString(e), c->exp_dtype, sy,
                sx, n_rects);
  return results_to_host(c, sums_out, c->iq_out.p, obytes);  // (synchronises: `rects` is read)
}

int kpdi_reduce_experimental(kpdi_ctx *c, int op, int axis_mask, int ny, int nx, void *out, size_t out_bytes) {
  int rc = check_patterns(c, "an axis reduction");
  if (rc) return rc;
  if (op < KPDI_REDUCE_SUM || op > KPDI_REDUCE_VAR) return fail(KPDI_EINVAL, "unknown reduction op %d", op);
  if (axis_mask < 1 || axis_mask > 15)
    return fail(KPDI_EINVAL, "axis mask %d: between 1 and 15, one bit per reduced axis of (ny, nx, sy, sx)", axis_mask);
  if (ny < 1 || nx < 1 || (int64_t)ny * nx != c->m_all)
    return fail(KPDI_EINVAL, "an axis reduction: a map of %d x %d points, %lld patterns are resident", ny, nx, (long long)c->m_all);
  if (!out) return fail(KPDI_EINVAL, "out is NULL");
  const kpdi::RedPlan plan = kpdi::reduce_plan(c->exp_dtype, op, axis_mask, ny, nx, c->sy, c->sx);
  if (plan.regime < 0)
    return fail(KPDI_EINVAL, "an axis reduction of %d x %d x %d x %d over the axes of mask %d: no kernel path takes this shape", ny, nx,
                c->sy, c->sx, axis_mask);
  const size_t obytes = (size_t)plan.n_out * plan.out_esize;
  if (out_bytes != obytes)
    return fail(KPDI_EINVAL, "out_bytes is %zu, the result has %lld values of %d bytes", out_bytes, (long long)plan.n_out, plan.out_esize);
  rc = start_pattern_op(c);
  if (rc) return rc;
  HIPCHK(c->red_ws.reserve(plan.workspace_bytes));
  kpdi::RedLaunch a{};
  a.patterns = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.ny = ny;
  a.nx = nx;
  a.sy = c->sy;
  a.sx = c->sx;
  a.op = op;
  a.axis_mask = axis_mask;
  a.workspace = c->red_ws.p;
  a.workspace_bytes = c->red_ws.cap;
  {
    kpdi::ScopedTimer t(c, &c->ev_pre);
    hipError_t e = kpdi::launch_reduce(a, c->stream);
    if (e != hipSuccess)
      return fail(KPDI_EHIP, "reduction kernel: %s (dtype %d, op %d, mask %d, %dx%dx%dx%d)", hipGetErrorString(e), c->exp_dtype, op,
                  axis_mask, ny, nx, c->sy, c->sx);
  }
  return results_to_host(c, out, (const char *)c->red_ws.p + plan.out_off, obytes);
}

int kpdi_reduce_plan_describe(int dtype, int op, int axis_mask, int ny, int nx, int sy, int sx, int64_t *desc) {
  if (!desc) return fail(KPDI_EINVAL, "desc is NULL");
  const kpdi::RedPlan p = kpdi::reduce_plan(dtype, op, axis_mask, ny, nx, sy, sx);
  if (p.regime < 0)
    return fail(KPDI_EINVAL, "an axis reduction of %d x %d x %d x %d of dtype %d with op %d over the axes of mask %d: no kernel path "
                             "takes it", ny, nx, sy, sx, dtype, op, axis_mask);
  const int64_t d[17] = {p.regime, p.sh.A, p.sh.R1, p.sh.M, p.sh.R2, p.sh.B, p.slice, p.n_slices, p.vec, p.group,
                         p.grid_x, p.grid_y, p.passes, p.planes, (int64_t)p.workspace_bytes, (int64_t)p.n_out * p.out_esize,
                         p.combine_lanes};
  std::copy(d, d + 17, desc);
  return KPDI_OK;
}

int kpdi_fft_filter(kpdi_ctx *c, int function_domain, const double *table, int ty, int tx) {
  int rc = check_patterns(c, "the FFT filter");
  if (rc) return rc;
  if (!table) return fail(KPDI_EINVAL, "table is NULL");
  const int sy = c->sy, sx = c->sx, h = kpdi::half_cols(sx);
  const bool freq = function_domain == KPDI_DOMAIN_FREQUENCY;
  if (!freq && function_domain != KPDI_DOMAIN_SPATIAL) return fail(KPDI_EINVAL, "unknown function domain %d", function_domain);
  if (freq && (ty != sy || tx != h))
    return fail(KPDI_EINVAL, "folded transfer function of %d x %d, patterns of %d x %d need %d x %d", ty, tx, sy, sx, sy, h);
  if (!freq && (ty < 1 || tx < 1 || (int64_t)ty * tx > (1 << 20)))
    return fail(KPDI_EINVAL, "spatial kernel of %d x %d", ty, tx);
  const kpdi::FfPlan plan =  // (what launch_fft_filter follows)
      kpdi::fft_filter_launch_plan(freq ? kpdi::FF_DOMAIN_FREQUENCY : kpdi::FF_DOMAIN_SPATIAL, sy, sx, c->m_all);
  if (plan.path < 0) return fail(KPDI_EINVAL, "FFT filter of %d x %d patterns: no kernel path takes this shape", sy, sx);
  rc = start_pattern_op(c);
  if (rc) return rc;
  // frequency: twiddles (f32) + the folded table / (sy sx) as f32 complex; spatial: the kernel rounded to f32, as doubles
  std::vector<char> tab;
  size_t tab_off = 0;
  if (freq) {
    const size_t tbytes = 2 * ((size_t)sx + sy) * sizeof(float), hbytes = 2 * (size_t)sy * h * sizeof(float);
    tab.resize(tbytes + hbytes);
    write_twiddles((float *)tab.data(), sy, sx);
    float *hs = (float *)(tab.data() + tbytes);
    const double scale = 1.0 / ((double)sy * sx);
    for (size_t i = 0; i < 2 * (size_t)sy * h; ++i) hs[i] = (float)(table[i] * scale);
    tab_off = tbytes;
  } else {
    tab.resize((size_t)ty * tx * sizeof(double));
    double *tp = (double *)tab.data();
    for (size_t i = 0; i < (size_t)ty * tx; ++i) tp[i] = (double)(float)table[i];
  }
  HIPCHK(c->op_tab.reserve(tab.size()));
  HIPCHK(hipMemcpyAsync(c->op_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, c->stream));
  if (plan.path == 1) HIPCHK(c->op_ws.reserve(plan.workspace_bytes));
  kpdi::FfLaunch a{};
  a.patterns = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.n = c->m_all;
  a.sy = sy;
  a.sx = sx;
  a.domain = freq ? kpdi::FF_DOMAIN_FREQUENCY : kpdi::FF_DOMAIN_SPATIAL;
  a.twiddles = freq ? (const float *)c->op_tab.p : nullptr;
  a.table = freq ? (const float *)((const char *)c->op_tab.p + tab_off) : nullptr;
  a.taps = freq ? nullptr : (const double *)c->op_tab.p;
  a.ty = ty;
  a.tx = tx;
  dtype_range(c->exp_dtype, &a.omin, &a.omax);
  a.workspace = c->op_ws.p;
  a.workspace_bytes = c->op_ws.cap;
  hipError_t e = kpdi::launch_fft_filter(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "FFT-filter kernel: %s (dtype %d, %dx%d)", hipGetErrorString(e), c->exp_dtype, sy, sx);
  HIPCHK(hipStreamSynchronize(c->stream));  // `tab` dies at scope exit
  patterns_changed(c);
  return KPDI_OK;
}

}  // extern "C"

namespace kpdi {

// common part of kpdi_rescale_intensity / kpdi_normalize_intensity: the recorded background steps first, then one
// kernel from exp_raw into exp_raw (same dtype) or into int_out, which then becomes exp_raw (a new dtype: converting in
// place would let one workgroup's writes overtake another's reads whenever the element size changes)
static int run_intensity(kpdi_ctx *c, IntLaunch &a) {
  int rc = check_patterns(c, "intensity rescaling");
  if (rc) return rc;
  if (!intensity_dtype(a.dtype_out)) return bad_dtype_out(a.dtype_out, "intensity rescaling writes");
  if (int_plan(c->exp_dtype, c->sy, c->sx, c->m_all).path < 0)
    return fail(KPDI_EINVAL, "intensity rescaling of %lld patterns of %d x %d: no kernel path takes this shape",
                (long long)c->m_all, c->sy, c->sx);
  rc = start_pattern_op(c);
  if (rc) return rc;
  const bool same = a.dtype_out == c->exp_dtype;
  if (!same) HIPCHK(c->int_out.reserve((size_t)c->m_all * c->npix * dtype_size(a.dtype_out)));
  a.src = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.dst = same ? c->exp_raw.p : c->int_out.p;
  a.n = c->m_all;
  a.sy = c->sy;
  a.sx = c->sx;
  hipError_t e = launch_intensity(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "intensity kernel: %s (dtype %d -> %d, %dx%d)", hipGetErrorString(e), c->exp_dtype,
                a.dtype_out, c->sy, c->sx);
  if (same) patterns_changed(c);
  else adopt_output(c, a.dtype_out);
  return KPDI_OK;
}

}  // namespace kpdi

extern "C" {

int kpdi_rescale_intensity(kpdi_ctx *c, const double *in_range, const double *percentiles, double omin, double omax,
                           int dtype_out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  if (in_range && percentiles) return fail(KPDI_EINVAL, "in_range and percentiles are exclusive");
  kpdi::IntLaunch a{};
  a.dtype_out = dtype_out;
  a.omin = omin;
  a.orange = omax - omin;
  if (percentiles) {
    a.mode = kpdi::INT_MODE_PERCENTILE;
    a.q0 = percentiles[0] / 100.0;  // np.true_divide(q, 100.0)
    a.q1 = percentiles[1] / 100.0;
    if (!(a.q0 >= 0 && a.q0 <= 1 && a.q1 >= 0 && a.q1 <= 1)) return fail(KPDI_EINVAL, "Percentiles must be in the range [0, 100]");
  } else if (in_range) {
    a.mode = kpdi::INT_MODE_RANGE;
    a.lo = in_range[0];
    a.hi = in_range[1];
  } else {
    a.mode = kpdi::INT_MODE_MINMAX;
  }
  return kpdi::run_intensity(c, a);
}

int kpdi_normalize_intensity(kpdi_ctx *c, double num_std, int divide_by_square_root, int dtype_out) {
  kpdi::IntLaunch a{};  // (run_intensity checks the context and the patterns first)
  a.dtype_out = dtype_out;
  a.mode = kpdi::INT_MODE_NORMALIZE;
  a.num_std = num_std;
  a.divide_by_square_root = divide_by_square_root != 0;
  return kpdi::run_intensity(c, a);
}

int kpdi_intensity_range(kpdi_ctx *c, double *out) {
  int rc = kpdi::check_patterns(c, "intensity rescaling");
  if (rc) return rc;
  if (!out) return fail(KPDI_EINVAL, "out is NULL");
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  HIPCHK(c->int_ws.reserve((3 * (size_t)kpdi::INT_RANGE_BLOCKS + 2) * sizeof(double)));
  double *ws = c->int_ws.as<double>();
  hipError_t e = kpdi::launch_intensity_range(c->exp_raw.p, c->exp_dtype, c->m_all * (int64_t)c->npix, ws + 2, ws,
                                              c->stream);
  if (e != hipSuccess) return fail(KPDI_EHIP, "intensity range kernel: %s", hipGetErrorString(e));
  return results_to_host(c, out, ws, 2 * sizeof(double));
}

int kpdi_adaptive_histogram_equalization(kpdi_ctx *c, int ky, int kx, int clip_count, int nbins) {
  int rc = kpdi::check_patterns(c, "adaptive histogram equalization");
  if (rc) return rc;
  if (ky < 1 || kx < 1) return fail(KPDI_EINVAL, "kernel of %d x %d", ky, kx);
  if (nbins < 1 || nbins > kpdi::CLAHE_MAX_NBINS) return fail(KPDI_EINVAL, "nbins %d outside [1, %d]", nbins, kpdi::CLAHE_MAX_NBINS);
  if (clip_count < 1) return fail(KPDI_EINVAL, "clip_count %d < 1", clip_count);
  const kpdi::ClahePlan plan = kpdi::clahe_launch_plan(c->exp_dtype, c->sy, c->sx, ky, kx, nbins, c->m_all);
  if (plan.path < 0)
    return fail(KPDI_EINVAL, "adaptive histogram equalization of %d x %d patterns with a %d x %d kernel and %d bins: no kernel path takes this shape",
                c->sy, c->sx, ky, kx, nbins);
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  if (plan.path == 1) HIPCHK(c->op_ws.reserve(plan.workspace_bytes));
  kpdi::ClaheLaunch a{};
  a.patterns = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.n = c->m_all;
  a.sy = c->sy;
  a.sx = c->sx;
  a.ky = ky;
  a.kx = kx;
  a.clip_count = clip_count;
  a.nbins = nbins;
  float omin, omax;
  dtype_range(c->exp_dtype, &omin, &omax);
  a.omin = omin;
  a.omax = omax;
  a.workspace = c->op_ws.p;
  a.workspace_bytes = c->op_ws.cap;
  hipError_t e = kpdi::launch_clahe(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "adaptive histogram equalization kernel: %s (dtype %d, %dx%d)", hipGetErrorString(e),
                c->exp_dtype, c->sy, c->sx);
  patterns_changed(c);
  return KPDI_OK;
}

}  // extern "C"

namespace kpdi {

// what both neighbour ops check: the resident patterns as a map of ny x nx points, the window, the output rows
static int check_neighbour_args(kpdi_ctx *c, const char *op, int ny, int nx, const void *window, int wy, int wx, int row0,
                                int row1) {
  int rc = check_patterns(c, op);
  if (rc) return rc;
  if (ny < 1 || nx < 1 || (int64_t)ny * nx != c->m_all)
    return fail(KPDI_EINVAL, "%s: a map of %d x %d points, %lld patterns are resident", op, ny, nx, (long long)c->m_all);
  if (!window || wy < 1 || wx < 1 || (int64_t)wy * wx > NB_MAX_WINDOW)
    return fail(KPDI_EINVAL, "%s: window of %d x %d", op, wy, wx);
  if (row0 < 0 || row1 > ny || row0 >= row1) return fail(KPDI_EINVAL, "%s: rows [%d, %d) of %d", op, row0, row1, ny);
  if ((int64_t)(row1 - row0) * nx > INT_MAX) return fail(KPDI_EINVAL, "%s: too many map points in one call", op);
  return KPDI_OK;
}

}  // namespace kpdi

extern "C" {

int kpdi_average_neighbour_patterns(kpdi_ctx *c, int ny, int nx, const double *window, int wy, int wx,
                                    const int64_t *window_sums, int row0, int row1) {
  int rc = kpdi::check_neighbour_args(c, "neighbour averaging", ny, nx, window, wy, wx, row0, row1);
  if (rc) return rc;
  if (!window_sums) return fail(KPDI_EINVAL, "window_sums is NULL");
  std::vector<kpdi::NbTap> taps;
  for (int j = 0; j < wy * wx; ++j) {
    if (!std::isfinite(window[j])) return fail(KPDI_EINVAL, "window coefficient %d is not finite", j);
    if (window[j] != 0.0) taps.push_back(kpdi::NbTap{window[j], j / wx - wy / 2, j % wx - wx / 2, j, 0});
  }
  const size_t n = (size_t)c->m_all;
  std::vector<double> ws(n);
  for (size_t i = 0; i < n; ++i) {
    ws[i] = (double)window_sums[i];
    if (window_sums[i] == 0 && i >= (size_t)row0 * nx && i < (size_t)row1 * nx)
      return fail(KPDI_EINVAL, "the window sum of map point %zu is 0: its average is undefined", i);
  }
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  const size_t tbytes = (taps.size() + 1) * sizeof(kpdi::NbTap), bytes = n * c->npix * kpdi::dtype_size(c->exp_dtype);
  HIPCHK(c->op_tab.reserve(tbytes + n * sizeof(double)));
  if (!taps.empty())
    HIPCHK(hipMemcpyAsync(c->op_tab.p, taps.data(), taps.size() * sizeof(kpdi::NbTap), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync((char *)c->op_tab.p + tbytes, ws.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c->int_out.reserve(bytes));
  kpdi::NbAvgLaunch a{};
  a.src = c->exp_raw.p;
  a.dst = c->int_out.p;
  a.dtype = c->exp_dtype;
  a.ny = ny;
  a.nx = nx;
  a.sy = c->sy;
  a.sx = c->sx;
  a.row0 = row0;
  a.row1 = row1;
  a.taps = (const kpdi::NbTap *)c->op_tab.p;
  a.ntaps = (int)taps.size();
  a.ws = (const double *)((const char *)c->op_tab.p + tbytes);
  float omin, omax;
  dtype_range(c->exp_dtype, &omin, &omax);
  a.omin = omin;
  a.orange = (double)omax - (double)omin;
  hipError_t e = kpdi::launch_neighbour_average(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "neighbour averaging kernel: %s (dtype %d, %dx%d)", hipGetErrorString(e), c->exp_dtype, c->sy, c->sx);
  // rows that are resident only as neighbours keep their patterns
  const size_t row_bytes = bytes / ny;
  if (row0 > 0)
    HIPCHK(hipMemcpyAsync(c->int_out.p, c->exp_raw.p, row_bytes * row0, hipMemcpyDeviceToDevice, c->stream));
  if (row1 < ny)
    HIPCHK(hipMemcpyAsync((char *)c->int_out.p + row_bytes * row1, (const char *)c->exp_raw.p + row_bytes * row1,
                          row_bytes * (ny - row1), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // `taps` and `ws` die at scope exit
  kpdi::adopt_output(c);
  return KPDI_OK;
}

int kpdi_neighbour_dot_products(kpdi_ctx *c, int ny, int nx, const uint8_t *footprint, int wy, int wx, int zero_mean,
                                int normalize, int f64, int row0, int row1, void *matrices_out, void *map_out) {
  int rc = kpdi::check_neighbour_args(c, "neighbour dot products", ny, nx, footprint, wy, wx, row0, row1);
  if (rc) return rc;
  if (!matrices_out && !map_out) return fail(KPDI_EINVAL, "matrices_out and map_out are both NULL");
  const int wsize = wy * wx, jorigin = (wy / 2) * wx + wx / 2;
  if (!footprint[jorigin]) return fail(KPDI_EINVAL, "the footprint is false at its own origin (%d, %d)", wy / 2, wx / 2);
  std::vector<kpdi::NbTap> taps;
  for (int j = 0; j < wsize; ++j)
    if (footprint[j] && j != jorigin) taps.push_back(kpdi::NbTap{1.0, j / wx - wy / 2, j % wx - wx / 2, j, 0});
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  const size_t n = (size_t)c->m_all, n_out = (size_t)(row1 - row0) * nx, esz = f64 ? 8 : 4;
  const size_t stats_bytes = n * 2 * sizeof(double), mat_bytes = matrices_out ? n_out * wsize * esz : 0;
  const size_t mat_off = stats_bytes, map_off = (mat_off + mat_bytes + 15) & ~(size_t)15;
  HIPCHK(c->op_tab.reserve((taps.size() + 1) * sizeof(kpdi::NbTap)));
  if (!taps.empty())
    HIPCHK(hipMemcpyAsync(c->op_tab.p, taps.data(), taps.size() * sizeof(kpdi::NbTap), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c->op_ws.reserve(map_off + n_out * esz));
  char *ws = (char *)c->op_ws.p;
  hipError_t e = kpdi::launch_neighbour_stats(c->exp_raw.p, c->exp_dtype, c->m_all, c->sy, c->sx, zero_mean ? 1 : 0,
                                              (double *)ws, c->stream);
  if (e != hipSuccess) return fail(KPDI_EHIP, "neighbour statistics kernel: %s", hipGetErrorString(e));
  kpdi::NbDotLaunch a{};
  a.src = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.ny = ny;
  a.nx = nx;
  a.sy = c->sy;
  a.sx = c->sx;
  a.row0 = row0;
  a.row1 = row1;
  a.taps = (const kpdi::NbTap *)c->op_tab.p;
  a.ntaps = (int)taps.size();
  a.wsize = wsize;
  a.jorigin = jorigin;
  a.stats = (const double2 *)ws;
  a.normalize = normalize ? 1 : 0;
  a.f64 = f64 ? 1 : 0;
  a.matrices = matrices_out ? ws + mat_off : nullptr;
  a.map = map_out ? ws + map_off : nullptr;
  e = kpdi::launch_neighbour_dot(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "neighbour dot product kernel: %s (dtype %d, %dx%d)", hipGetErrorString(e), c->exp_dtype, c->sy, c->sx);
  if (matrices_out) {
    rc = results_to_host(c, matrices_out, a.matrices, mat_bytes);
    if (rc) return rc;
  }
  if (map_out) return results_to_host(c, map_out, a.map, n_out * esz);
  return KPDI_OK;  // (results_to_host synchronised: `taps` may die)
}

int kpdi_downsample(kpdi_ctx *c, int factor, int dtype_out) {
  int rc = kpdi::check_patterns(c, "downsampling");
  if (rc) return rc;
  if (!kpdi::intensity_dtype(dtype_out)) return kpdi::bad_dtype_out(dtype_out, "downsampling writes");
  const int sy = c->sy, sx = c->sx;
  if (factor < 2) return fail(KPDI_EINVAL, "binning factor %d must be an integer > 1", factor);
  if (sy % factor || sx % factor)
    return fail(KPDI_EINVAL, "binning factor %d must divide the detector shape (%d, %d)", factor, sy, sx);
  if (c->have_sig_mask)
    return fail(KPDI_EINVAL, "a signal mask is set for the %d x %d detector: call kpdi_set_problem without it, downsample, "
                             "then set the mask of the binned shape", sy, sx);
  if (!c->held.empty() || c->pending_hold.rows > 0)
    return fail(KPDI_EINVAL, "dictionary chunks are held for the %d x %d detector: release them before downsampling", sy, sx);
  const kpdi::DsPlan plan = kpdi::downsample_launch_plan(c->exp_dtype, sy, sx, factor, c->m_all);
  if (plan.path < 0)
    return fail(KPDI_EINVAL, "downsampling of %d x %d patterns by %d: no kernel path takes this shape", sy, sx, factor);
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  const int ny = sy / factor, nx = sx / factor;
  HIPCHK(c->int_out.reserve((size_t)c->m_all * ny * nx * kpdi::dtype_size(dtype_out)));
  if (plan.path == 1) HIPCHK(c->op_ws.reserve(plan.workspace_bytes));
  kpdi::DsLaunch a{};
  a.src = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.dst = c->int_out.p;
  a.dtype_out = dtype_out;
  a.n = c->m_all;
  a.sy = sy;
  a.sx = sx;
  a.factor = factor;
  kpdi::dtype_range(dtype_out, &a.omin, &a.omax);
  a.workspace = c->op_ws.p;
  a.workspace_bytes = c->op_ws.cap;
  hipError_t e = kpdi::launch_downsample(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "downsampling kernel: %s (dtype %d -> %d, %dx%d by %d)", hipGetErrorString(e), c->exp_dtype,
                dtype_out, sy, sx, factor);
  // the problem follows the patterns: the binned detector without a signal mask; metric, arithmetic and keep_n stay
  // (there are no held chunks to release)
  kpdi::set_detector_layout(c, ny, nx, false, {});
  kpdi::adopt_output(c, dtype_out);
  return KPDI_OK;
}

int kpdi_get_dynamic_background(kpdi_ctx *c, int filter_domain, double std, double truncate, int dtype_out, void *out) {
  int rc = kpdi::check_patterns(c, "the dynamic background");
  if (rc) return rc;
  if (!out) return fail(KPDI_EINVAL, "out is NULL");
  if (!kpdi::intensity_dtype(dtype_out)) return kpdi::bad_dtype_out(dtype_out, "the dynamic background is written as");
  if (std <= 0) std = c->sx / 8.0;  // signals/ebsd.py:741-742
  std::vector<double> taps;
  int n, centre, reflect;
  rc = kpdi::gaussian_taps(filter_domain, std, truncate, taps, &n, &centre, &reflect);
  if (rc) return rc;
  const size_t sbytes = kpdi::dynamic_background_scratch_bytes(c->sy, c->sx, c->m_all, nullptr);
  if (sbytes == 0)
    return fail(KPDI_EINVAL, "the dynamic background of %d x %d patterns: no kernel path takes this shape", c->sy, c->sx);
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  rc = kpdi::upload_taps(c, taps);
  if (rc) return rc;
  const size_t obytes = (size_t)c->m_all * c->npix * kpdi::dtype_size(dtype_out);
  HIPCHK(c->int_out.reserve(obytes));
  HIPCHK(c->op_ws.reserve(sbytes));
  kpdi::DbLaunch a{};
  a.src = c->exp_raw.p;
  a.dtype = c->exp_dtype;
  a.dst = c->int_out.p;
  a.dtype_out = dtype_out;
  a.n = c->m_all;
  a.sy = c->sy;
  a.sx = c->sx;
  a.taps_padded = c->taps.as<double>();
  a.ntaps = n;
  a.centre = centre;
  a.spatial = reflect;
  a.scratch = (double *)c->op_ws.p;
  a.scratch_bytes = c->op_ws.cap;
  hipError_t e = kpdi::launch_dynamic_background(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "dynamic background kernel: %s (dtype %d -> %d, %dx%d)", hipGetErrorString(e), c->exp_dtype,
                dtype_out, c->sy, c->sx);
  return kpdi::results_to_host(c, out, c->int_out.p, obytes);
}

}  // extern "C"

namespace kpdi {

// what the decomposition calls share once their own arguments are checked: the plan of the resident set (refused above
// DEC_MAX_SIDE), the recorded background steps, and the means that `centre` removes, left in c->dec_mean
static int start_decomposition(kpdi_ctx *c, int centre, DecPlan *plan, DecLaunch *a) {
  if (centre != DEC_CENTRE_NONE && centre != DEC_CENTRE_NAVIGATION && centre != DEC_CENTRE_SIGNAL)
    return fail(KPDI_EINVAL, "centre %d: 0 (none), 1 (\"navigation\") or 2 (\"signal\")", centre);
  *plan = dec_plan(c->m_all, c->npix);
  if (plan->too_large)
    return fail(KPDI_EINVAL, "decomposition of %lld patterns of %d pixels: the Gram matrix would have %lld rows, above the "
                             "limit of %lld (it is solved on the host); bin the patterns first (downsample)",
                (long long)c->m_all, c->npix, (long long)plan->side, (long long)DEC_MAX_SIDE);
  if (!plan->ok) return fail(KPDI_EINVAL, "decomposition of %lld patterns of %d pixels: no kernel takes this shape",
                             (long long)c->m_all, c->npix);
  int rc = start_pattern_op(c);
  if (rc) return rc;
  *a = DecLaunch{};
  a->patterns = c->exp_raw.p;
  a->dtype = c->exp_dtype;
  a->m = c->m_all;
  a->k = c->npix;
  a->centre = centre;
  if (centre == DEC_CENTRE_NONE) return KPDI_OK;
  const size_t n_mean = centre == DEC_CENTRE_SIGNAL ? (size_t)a->m : (size_t)a->k;
  const size_t n_part = centre == DEC_CENTRE_NAVIGATION ? (size_t)dec_mean_chunks(a->m) * (size_t)a->k : 0;
  HIPCHK(c->dec_mean.reserve((n_mean + n_part) * sizeof(double)));
  a->mean = c->dec_mean.as<double>();
  a->mean_partial = n_part ? a->mean + n_mean : nullptr;
  hipError_t e = launch_decomposition_means(*a, c->stream);
  if (e != hipSuccess) return fail(KPDI_EHIP, "decomposition means kernel: %s", hipGetErrorString(e));
  return KPDI_OK;
}

}  // namespace kpdi

extern "C" {

int kpdi_decomposition_gram(kpdi_ctx *c, int centre, double *gram_out, double *mean_out, int64_t *side, int *transposed) {
  int rc = kpdi::check_patterns(c, "decomposition");
  if (rc) return rc;
  if (!gram_out || !side || !transposed) return fail(KPDI_EINVAL, "gram_out, side or transposed is NULL");
  kpdi::DecPlan plan;
  kpdi::DecLaunch a;
  rc = kpdi::start_decomposition(c, centre, &plan, &a);
  if (rc) return rc;
  const size_t n = (size_t)plan.side;
  HIPCHK(c->dec_out.reserve(n * n * sizeof(double)));
  hipError_t e = kpdi::launch_decomposition_gram(a, plan.transposed, c->dec_out.as<double>(), c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "decomposition Gram kernel: %s (dtype %d, %lld x %d)", hipGetErrorString(e), c->exp_dtype,
                (long long)c->m_all, c->npix);
  rc = kpdi::results_to_host(c, gram_out, c->dec_out.p, n * n * sizeof(double));
  if (rc) return rc;
  if (mean_out && centre != kpdi::DEC_CENTRE_NONE) {
    rc = kpdi::results_to_host(c, mean_out, a.mean, (size_t)(centre == kpdi::DEC_CENTRE_SIGNAL ? a.m : a.k) * sizeof(double));
    if (rc) return rc;
  }
  *side = plan.side;
  *transposed = plan.transposed;
  double trace = 0;
  for (size_t i = 0; i < n; ++i) trace += gram_out[i * n + i];
  if (!std::isfinite(trace)) return fail(KPDI_EINVAL, "patterns hold non-finite values: the trace of the Gram matrix is not finite");
  return KPDI_OK;
}

int kpdi_decomposition_apply(kpdi_ctx *c, int centre, int transposed_op, const double *basis, int n_components, double *out) {
  int rc = kpdi::check_patterns(c, "decomposition");
  if (rc) return rc;
  if (!basis || !out) return fail(KPDI_EINVAL, "basis or out is NULL");
  if (transposed_op != 0 && transposed_op != 1) return fail(KPDI_EINVAL, "transposed_op %d: 0 (Xc basis) or 1 (Xc^T basis)", transposed_op);
  const int64_t side = c->m_all < c->npix ? c->m_all : c->npix;
  if (n_components < 1 || n_components > side)
    return fail(KPDI_EINVAL, "%d components: between 1 and min(patterns, pixels) = %lld", n_components, (long long)side);
  kpdi::DecPlan plan;
  kpdi::DecLaunch a;
  rc = kpdi::start_decomposition(c, centre, &plan, &a);
  if (rc) return rc;
  const size_t in_rows = transposed_op ? (size_t)a.m : (size_t)a.k, out_rows = transposed_op ? (size_t)a.k : (size_t)a.m;
  const size_t in_bytes = in_rows * n_components * sizeof(double), out_bytes = out_rows * n_components * sizeof(double);
  HIPCHK(c->dec_in.reserve(in_bytes));
  HIPCHK(c->dec_out.reserve(out_bytes));
  HIPCHK(hipMemcpyAsync(c->dec_in.p, basis, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipError_t e = kpdi::launch_decomposition_apply(a, transposed_op, c->dec_in.as<double>(), n_components, c->dec_out.as<double>(),
                                                  c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "decomposition apply kernel: %s (dtype %d, %lld x %d, %d components)", hipGetErrorString(e),
                c->exp_dtype, (long long)c->m_all, c->npix, n_components);
  return kpdi::results_to_host(c, out, c->dec_out.p, out_bytes);  // (synchronises: `basis` is read)
}

int kpdi_decomposition_model(kpdi_ctx *c, const void *loadings, const void *factors, int n_components, const double *mean,
                             int mean_kind, int dtype_out) {
  int rc = kpdi::check_patterns(c, "the decomposition model");
  if (rc) return rc;
  if (!loadings || !factors) return fail(KPDI_EINVAL, "loadings or factors is NULL");
  if (dtype_out != KPDI_F32 && dtype_out != KPDI_F64)
    return fail(KPDI_EINVAL, "dtype_out %d: the decomposition model is written as float32 or float64", dtype_out);
  if (mean && mean_kind != kpdi::DEC_CENTRE_NAVIGATION && mean_kind != kpdi::DEC_CENTRE_SIGNAL)
    return fail(KPDI_EINVAL, "mean_kind %d: 1 (a mean per pixel) or 2 (a mean per pattern)", mean_kind);
  const int64_t side = c->m_all < c->npix ? c->m_all : c->npix;
  if (n_components < 1 || n_components > side)
    return fail(KPDI_EINVAL, "%d components: between 1 and min(patterns, pixels) = %lld", n_components, (long long)side);
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  const size_t es = kpdi::dtype_size(dtype_out), m = (size_t)c->m_all, k = (size_t)c->npix;
  const size_t n_mean = !mean ? 0 : mean_kind == kpdi::DEC_CENTRE_SIGNAL ? m : k;
  HIPCHK(c->dec_in.reserve(m * n_components * es));
  HIPCHK(c->dec_in2.reserve(k * n_components * es));
  HIPCHK(c->int_out.reserve(m * k * es));
  HIPCHK(hipMemcpyAsync(c->dec_in.p, loadings, m * n_components * es, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->dec_in2.p, factors, k * n_components * es, hipMemcpyHostToDevice, c->stream));
  if (n_mean) {
    HIPCHK(c->dec_mean.reserve(n_mean * sizeof(double)));
    HIPCHK(hipMemcpyAsync(c->dec_mean.p, mean, n_mean * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  kpdi::DecModelLaunch a{};
  a.loadings = c->dec_in.p;
  a.factors = c->dec_in2.p;
  a.m = c->m_all;
  a.k = c->npix;
  a.c = n_components;
  a.mean = n_mean ? c->dec_mean.as<double>() : nullptr;
  a.mean_kind = mean_kind;
  a.dst = c->int_out.p;
  a.dtype_out = dtype_out;
  hipError_t e = kpdi::launch_decomposition_model(a, c->stream);
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "decomposition model kernel: %s (%lld x %d, %d components)", hipGetErrorString(e), (long long)c->m_all,
                c->npix, n_components);
  HIPCHK(hipStreamSynchronize(c->stream));  // the caller's arrays are read
  kpdi::adopt_output(c, dtype_out);
  return KPDI_OK;
}

int kpdi_change_dtype(kpdi_ctx *c, int dtype_out) {
  int rc = kpdi::check_patterns(c, "a dtype change");
  if (rc) return rc;
  if (!kpdi::intensity_dtype(dtype_out)) return kpdi::bad_dtype_out(dtype_out, "patterns are cast to");
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  if (dtype_out == c->exp_dtype) return KPDI_OK;
  const int64_t count = c->m_all * (int64_t)c->npix;
  HIPCHK(c->int_out.reserve((size_t)count * kpdi::dtype_size(dtype_out)));
  hipError_t e = kpdi::launch_change_dtype(c->exp_raw.p, c->exp_dtype, c->int_out.p, dtype_out, count, c->stream);
  if (e != hipSuccess) return fail(KPDI_EHIP, "dtype change kernel: %s (dtype %d -> %d)", hipGetErrorString(e), c->exp_dtype, dtype_out);
  kpdi::adopt_output(c, dtype_out);
  return KPDI_OK;
}

}  // extern "C"

namespace kpdi {

// what kpdi_select_patterns was asked for, checked against the source detector
struct SelRequest {
  const int64_t *index;  // host, or nullptr (identity)
  int64_t n_out;
  int row0, row_step, n_rows, col0, col_step, n_cols;
  bool moves(const kpdi_ctx *c) const {  // does anything but "every pattern, whole, in order"
    return index || row0 || col0 || row_step != 1 || col_step != 1 || n_rows != c->sy || n_cols != c->sx;
  }
};

// the selection kernel on c's stream, from `from` (patterns of sy x sx elements of `esize` bytes) into `to`; the index
// list goes up first
static int run_select(kpdi_ctx *c, const void *from, void *to, int esize, int sy, int sx, const SelRequest &r) {
  kpdi::SelLaunch a{};
  if (r.index) {
    const size_t bytes = (size_t)r.n_out * sizeof(int64_t);
    HIPCHK(c->sel_idx.reserve(bytes));
    HIPCHK(hipMemcpyAsync(c->sel_idx.p, r.index, bytes, hipMemcpyHostToDevice, c->stream));
    c->cnt.h2d_bytes += (double)bytes;
    a.index = c->sel_idx.as<int64_t>();
  }
  a.src = from;
  a.dst = to;
  a.n_out = r.n_out;
  a.esize = esize;
  a.sy = sy;
  a.sx = sx;
  a.row0 = r.row0;
  a.row_step = r.row_step;
  a.n_rows = r.n_rows;
  a.col0 = r.col0;
  a.col_step = r.col_step;
  a.n_cols = r.n_cols;
  {
    ScopedTimer t(c, &c->ev_pre);
    hipError_t e = kpdi::launch_select(a, c->stream);
    if (e != hipSuccess)
      return fail(KPDI_EHIP, "selection kernel: %s (%d-byte elements, %dx%d -> %dx%d)", hipGetErrorString(e), esize, sy, sx,
                  r.n_rows, r.n_cols);
  }
  if (r.index) HIPCHK(hipStreamSynchronize(c->stream));  // the caller's list is read
  return KPDI_OK;
}

// c's resident patterns are now `n` patterns without a navigation mask
static int adopt_selection(kpdi_ctx *c, int64_t n) {
  c->m_all = n;
  int rc = set_navigation_mask(c, nullptr);
  if (rc) return rc;
  patterns_changed(c);
  return KPDI_OK;
}

// the selection replaces c's resident patterns: a gather cannot run in place, so it goes through int_out
static int select_in_place(kpdi_ctx *c, const SelRequest &r) {
  int rc = start_pattern_op(c);
  if (rc) return rc;
  if (r.moves(c)) {
    const int es = (int)kpdi::dtype_size(c->exp_dtype);
    HIPCHK(c->int_out.reserve((size_t)r.n_out * r.n_rows * r.n_cols * es));
    rc = run_select(c, c->exp_raw.p, c->int_out.p, es, c->sy, c->sx, r);
    if (rc) return rc;
    std::swap(c->exp_raw, c->int_out);
    if (r.n_rows != c->sy || r.n_cols != c->sx) kpdi::set_detector_layout(c, r.n_rows, r.n_cols, false, {});
  }
  return adopt_selection(c, r.n_out);
}

// the selection of src's patterns AS THEY ARE IN HBM (recorded steps not applied) becomes dst's resident set, on dst's
// stream; src's stream is idle.  dst takes the selection's shape as its problem (metric, arithmetic and keep_n of src)
// unless it already has a problem of that shape.
static int select_into(kpdi_ctx *src, kpdi_ctx *dst, const SelRequest &r) {
  dst->pend = kpdi_ctx::PendingPre{};  // recorded steps belonged to the previous set
  if (!dst->have_problem || dst->sy != r.n_rows || dst->sx != r.n_cols) {
    dst->have_exp = false;
    int rc = kpdi_set_problem(dst, r.n_rows, r.n_cols, nullptr, src->metric, src->exact64 ? KPDI_COMPUTE_F64 : src->compute,
                              src->keep_n);
    if (rc) return rc;
  }
  const int es = (int)kpdi::dtype_size(src->exp_dtype);
  HIPCHK(dst->exp_raw.reserve((size_t)r.n_out * r.n_rows * r.n_cols * es));
  int rc = run_select(dst, src->exp_raw.p, dst->exp_raw.p, es, src->sy, src->sx, r);
  if (rc) return rc;
  dst->exp_dtype = src->exp_dtype;
  dst->have_exp = true;
  rc = adopt_selection(dst, r.n_out);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(dst->stream));  // src may change its patterns as soon as this returns
  return KPDI_OK;
}

}  // namespace kpdi

extern "C" {

int kpdi_select_patterns(kpdi_ctx *src, kpdi_ctx *dst, const int64_t *pattern_index, int64_t n_out, int row0, int row_step,
                         int n_rows, int col0, int col_step, int n_cols) {
  if (!dst) return fail(KPDI_EINVAL, "dst is NULL");
  int rc = kpdi::check_patterns(src, "a selection");
  if (rc) return rc;
  const int sy = src->sy, sx = src->sx;
  if (n_out < 1 || n_out >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "a selection of %lld patterns", (long long)n_out);
  if (row_step < 1 || col_step < 1) return fail(KPDI_EINVAL, "steps (%d, %d) must be >= 1", row_step, col_step);
  if (!kpdi::sel_range_ok(row0, row_step, n_rows, sy))
    return fail(KPDI_EINVAL, "%d rows from row %d in steps of %d leave the %d x %d detector", n_rows, row0, row_step, sy, sx);
  if (!kpdi::sel_range_ok(col0, col_step, n_cols, sx))
    return fail(KPDI_EINVAL, "%d columns from column %d in steps of %d leave the %d x %d detector", n_cols, col0, col_step, sy,
                sx);
  if (!pattern_index && n_out != src->m_all)
    return fail(KPDI_EINVAL, "without an index list n_out = %lld must be the number of resident patterns, %lld",
                (long long)n_out, (long long)src->m_all);
  if (pattern_index)
    for (int64_t i = 0; i < n_out; ++i)
      if (pattern_index[i] < 0 || pattern_index[i] >= src->m_all)
        return fail(KPDI_EINVAL, "pattern_index[%lld] = %lld is outside [0, %lld)", (long long)i, (long long)pattern_index[i],
                    (long long)src->m_all);
  const int es = (int)kpdi::dtype_size(src->exp_dtype);
  if (kpdi::select_plan(es, sy, sx, n_out, row0, row_step, n_rows, col0, col_step, n_cols).path < 0)
    return fail(KPDI_EINVAL, "selection from %d x %d patterns: no kernel path takes this shape", sy, sx);
  if (dst != src && dst->device != src->device)
    return fail(KPDI_EINVAL, "the contexts are on devices %d and %d: a selection stays on one device", src->device, dst->device);
  const kpdi::SelRequest req{pattern_index, n_out, row0, row_step, n_rows, col0, col_step, n_cols};
  // recorded steps run before the selection.  Into another context they run THERE, on a copy of the whole set (src keeps
  // its patterns and its steps as they are), so dst passes through src's shape on its way
  const bool via_copy = dst != src && (src->pend.st || src->pend.dy) && req.moves(src);
  if (dst->have_problem) {
    const bool reshaped = dst->sy != n_rows || dst->sx != n_cols || (via_copy && (dst->sy != sy || dst->sx != sx));
    if (reshaped && dst->have_sig_mask)
      return fail(KPDI_EINVAL, "a signal mask is set for the %d x %d detector: call kpdi_set_problem without it, select, then "
                               "set the mask of the new shape", dst->sy, dst->sx);
    if (reshaped && (!dst->held.empty() || dst->pending_hold.rows > 0))
      return fail(KPDI_EINVAL, "dictionary chunks are held for the %d x %d detector: release them before selecting", dst->sy,
                  dst->sx);
  }
  rc = use_device(src);
  if (rc) return rc;
  if (dst == src) return kpdi::select_in_place(src, req);
  rc = use_device(dst);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(src->stream));  // dst's stream reads what src's wrote
  if (!src->pend.st && !src->pend.dy) return kpdi::select_into(src, dst, req);
  // every pattern, whole, with the recorded steps: they run when dst's patterns are next needed (or right below)
  const kpdi::SelRequest all{nullptr, src->m_all, 0, 1, sy, 0, 1, sx};
  // a dst that already has a problem of the selection's shape keeps its metric, arithmetic and keep_n (kpdi.h): the
  // detour through src's shape below takes src's, so they are put back at the end (no signal mask can be lost: with
  // one, a dst whose shape differs from src's was refused above)
  const bool own_problem = via_copy && dst->have_problem && dst->sy == n_rows && dst->sx == n_cols && (sy != n_rows || sx != n_cols);
  const int own_metric = dst->metric, own_compute = dst->exact64 ? KPDI_COMPUTE_F64 : dst->compute, own_keep_n = dst->keep_n;
  rc = kpdi::select_into(src, dst, all);
  if (rc) return rc;
  dst->pend = src->pend;
  if (src->pend.st) {
    HIPCHK(dst->bg.reserve((size_t)src->npix * sizeof(float)));
    HIPCHK(hipMemcpyAsync(dst->bg.p, src->bg.p, (size_t)src->npix * sizeof(float), hipMemcpyDeviceToDevice, dst->stream));
  }
  if (src->pend.dy) {
    HIPCHK(dst->taps.reserve(src->taps.cap));
    HIPCHK(hipMemcpyAsync(dst->taps.p, src->taps.p, src->taps.cap, hipMemcpyDeviceToDevice, dst->stream));
  }
  HIPCHK(hipStreamSynchronize(dst->stream));
  if (!via_copy) return KPDI_OK;
  rc = kpdi::select_in_place(dst, req);
  if (rc || !own_problem) return rc;
  return kpdi_set_problem(dst, n_rows, n_cols, nullptr, own_metric, own_compute, own_keep_n);  // (keeps the patterns)
}

int kpdi_set_navigation_mask(kpdi_ctx *c, const uint8_t *nav_mask) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  // recorded background steps run now, on their own: the sweep that follows then prepares from the STORED patterns, as
  // it does after an upload of processed patterns, with the same preparation kernel (the preparation fused into the
  // background kernel sums a pattern in another order: float patterns would score differently in the last bits)
  int rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  rc = kpdi::set_navigation_mask(c, nav_mask);
  if (rc) return rc;
  kpdi::patterns_changed(c);
  return KPDI_OK;
}

}  // extern "C"
