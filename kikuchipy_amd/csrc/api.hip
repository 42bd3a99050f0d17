// api.hip - host side of libkpdi.so, core: the C ABI of include/kpdi.h for a context's life cycle, the problem and the
// experimental set, the background-removal calls, device buffers and counters - on top of the kernels in prep.hip /
// preproc.hip.  The sweep itself lives in sweep.hip, float64 arithmetic in exact64.hip, the hand-over of the result and
// the communicators in finalize.hip, dictionary generation / refinement / OSM in extras.hip (split in round 5; they
// share context.h).
#include "context.h"

using namespace kpdi;

namespace {
thread_local std::string g_err;
}

namespace kpdi {

int fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// for the translation units that do not include context.h (group.hip, h5ebsd.hip)
int fail_msg(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return fail(code, "%s", buf);
}

const char *thread_error() { return g_err.c_str(); }

int drain_events(kpdi_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> &list, double *ms_sum) {
  for (auto &pr : list) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, pr.first, pr.second));
    *ms_sum += ms;
    c->ev_pool.push_back(pr.first);
    c->ev_pool.push_back(pr.second);
  }
  list.clear();
  return KPDI_OK;
}

// the copies of the last result (finalize_enqueue) read the running lists: whoever writes those next waits for them
int wait_result_copy(kpdi_ctx *c) {
  if (c->result_copy) {
    HIPCHK(hipStreamWaitEvent(c->stream, c->result_copy, 0));
    c->result_copy = nullptr;
  }
  return KPDI_OK;
}

// ---- queued initialisations: one launch (kernels.h: FillSegments) instead of one per buffer
int flush_fills(kpdi_ctx *c) {
  if (c->fills.n == 0) return KPDI_OK;
  {
    ScopedTimer t(c, &c->ev_fixed);
    HIPCHK(kpdi::launch_fill_segments(c->fills, c->stream));
  }
  c->fills.n = 0;
  return KPDI_OK;
}
int queue_fill(kpdi_ctx *c, void *p, size_t words, unsigned value, int bound_used) {
  if (words == 0) return KPDI_OK;
  if (c->fills.n == kpdi::FILL_SEGMENTS) {
    int rc = flush_fills(c);
    if (rc) return rc;
  }
  const int i = c->fills.n++;
  c->fills.p[i] = (unsigned *)p;
  c->fills.words[i] = words;
  c->fills.value[i] = value;
  c->fills.bound_used[i] = bound_used;
  return KPDI_OK;
}
constexpr unsigned BITS_NEG_INF = 0xff800000u, BITS_INT_MAX = 0x7fffffffu;
int queue_fill_topk(kpdi_ctx *c, float *scores, int *idx, size_t n) {
  int rc = queue_fill(c, scores, n, BITS_NEG_INF);
  return rc ? rc : queue_fill(c, idx, n, BITS_INT_MAX);
}

void dtype_range(int dtype, float *omin, float *omax) {
  // skimage.util.dtype.dtype_range, as used at signals/ebsd.py:523 and :676
  switch (dtype) {
    case KPDI_U8: *omin = 0.f; *omax = 255.f; break;
    case KPDI_U16: *omin = 0.f; *omax = 65535.f; break;
    case KPDI_I8: *omin = -128.f; *omax = 127.f; break;
    case KPDI_I16: *omin = -32768.f; *omax = 32767.f; break;
    default: *omin = -1.f; *omax = 1.f; break;  // float32 / float64
  }
}

// what the prep kernels are told: `ndp` is evaluated in its centred form (prep.hip) except in the
// first thing every entry point does.  `keep_pending`: the one caller (kpdi_push_dictionary_chunk) that starts its upload
// BEFORE it looks at the float64 certification of the previous chunk
int use_device(kpdi_ctx *c, bool keep_pending) {
  HIPCHK(hipSetDevice(c->device));
  if (c->pend64.active && !keep_pending) return resolve_exact64(c);
  return KPDI_OK;
}

static int set_experimental_common(kpdi_ctx *c, const void *src, bool src_on_device, int dtype, int64_t m_all,
                            const uint8_t *nav_mask) {
  if (!c->have_problem) return fail(KPDI_EINVAL, "kpdi_set_problem must be called before kpdi_set_experimental");
  const size_t es = kpdi::dtype_size(dtype);
  if (es == 0) return fail(KPDI_EINVAL, "unknown dtype %d", dtype);
  if (m_all <= 0) return fail(KPDI_EINVAL, "need at least one experimental pattern");
  if (!src) return fail(KPDI_EINVAL, "patterns pointer is NULL");
  const size_t bytes = (size_t)m_all * c->npix * es;
  HIPCHK(c->exp_raw.reserve(bytes));
  HIPCHK(hipMemcpyAsync(c->exp_raw.p, src, bytes, src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                        c->stream));
  if (!src_on_device) c->cnt.h2d_bytes += (double)bytes;
  c->exp_dtype = dtype;
  c->m_all = m_all;
  c->have_nav_mask = nav_mask != nullptr;
  c->pend = kpdi_ctx::PendingPre{};  // recorded steps belonged to the previous set
  if (nav_mask) {
    if (m_all >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "too many experimental patterns");
    std::vector<int> rows, inv((size_t)m_all, -1);  // kept pattern -> source row; source row -> kept pattern or -1
    rows.reserve((size_t)m_all);
    for (int64_t i = 0; i < m_all; ++i)
      if (!nav_mask[i]) {
        inv[(size_t)i] = (int)rows.size();
        rows.push_back((int)i);
      }
    c->m = (int)rows.size();
    HIPCHK(c->row_map.reserve(std::max<size_t>(rows.size(), 1) * sizeof(int)));
    HIPCHK(c->inv_map.reserve(inv.size() * sizeof(int)));
    if (!rows.empty())
      HIPCHK(hipMemcpyAsync(c->row_map.p, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->inv_map.p, inv.data(), inv.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // `rows` / `inv` die at scope exit
  } else {
    if (m_all >= (int64_t)INT_MAX) return fail(KPDI_EINVAL, "too many experimental patterns");
    c->m = (int)m_all;
  }
  c->m_pad = kpdi::round_up(std::max(c->m, 1), kpdi::TILE_EXP);
  c->have_exp = true;
  c->exp_prepared = false;
  c->run_valid = false;
  discard_pending(c);
  c->final_valid = false;
  return KPDI_OK;
}

// device -> caller's (pageable) buffer through the page-locked staging buffer, then synchronise
int results_to_host(kpdi_ctx *c, void *dst, const void *d_src, size_t bytes) {
  if (bytes == 0) {
    HIPCHK(hipStreamSynchronize(c->stream));
    return KPDI_OK;
  }
  if (c->pin_out.reserve(bytes) != hipSuccess) {  // no page-locked memory to be had: copy directly
    (void)hipGetLastError();
    HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return KPDI_OK;
  }
  HIPCHK(hipMemcpyAsync(c->pin_out.p, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(dst, c->pin_out.p, bytes);
  return KPDI_OK;
}

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

// (cos, sin)(2 pi j / n) as f32 pairs for j < sx, then for j < sy: 2 (sx + sy) floats
static void write_twiddles(float *tw, int sy, int sx) {
  for (int n : {sx, sy})
    for (int j = 0; j < n; ++j, tw += 2) {
      const double a = 2.0 * M_PI * j / n;
      tw[0] = (float)cos(a);
      tw[1] = (float)sin(a);
    }
}

}  // namespace kpdi

namespace kpdi {

// what of the problem depends on the detector shape and the signal mask (`keep`: the kept pixels, empty without a mask):
// the pixel counts and the floats per prepared row, for the metric and arithmetic already set in the context.  Shared by
// kpdi_set_problem and kpdi_downsample, which moves the problem to the binned detector.
static void set_detector_layout(kpdi_ctx *c, int sy, int sx, bool have_mask, std::vector<int> keep) {
  c->sy = sy;
  c->sx = sx;
  c->npix = sy * sx;
  c->have_sig_mask = have_mask;
  if (!have_mask) c->have_quad_desc = false;
  c->k_kept = have_mask ? (int)keep.size() : c->npix;
  c->kept_pixels = std::move(keep);
  // floats per prepared row; the float16 form packs two pixels into one float: steps of 48 pixels
  // (match16.hip).  `ndp` rows carry one extra column (prep.hip: centred evaluation), except in the float16 form
  c->kpad = c->compute == KPDI_COMPUTE_F16
                ? kpdi::round_up(c->k_kept, kpdi::f16_geometry(c->f16_waves).step) / 2
                : kpdi::round_up(c->k_kept + (c->metric == KPDI_METRIC_NDP ? 1 : 0),
                                 c->wide32 ? kpdi::F16_STEP / 2 : kpdi::TILE_K);
  c->cnt.kpad = c->kpad;
  c->cnt.k_kept = c->k_kept;
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

const char *kpdi_version(void) { return "kpdi 0.13.0 (gfx950)"; }

size_t kpdi_counters_size(void) { return sizeof(kpdi_counters); }

const char *kpdi_last_error(void) { return g_err.c_str(); }

int kpdi_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int kpdi_create(int device_id, kpdi_ctx **out) {
  if (!out) return fail(KPDI_EINVAL, "out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    return fail(KPDI_ENODEV, "no HIP device visible: libkpdi has no CPU fallback");
  if (device_id < 0 || device_id >= n) return fail(KPDI_EINVAL, "device %d out of range [0, %d)", device_id, n);
  HIPCHK(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(KPDI_ENODEV, "device %d is %s; libkpdi is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
  kpdi_ctx *c = new kpdi_ctx();
  c->device = device_id;
  c->n_cu = prop.multiProcessorCount;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(KPDI_EHIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
  }
  *out = c;
  return KPDI_OK;
}

int kpdi_destroy(kpdi_ctx *c) {
  if (!c) return KPDI_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
  release_held(c);
  for (auto &st : c->rot_stage)
    if (st.copied) (void)hipEventDestroy(st.copied);
  if (c->pend64.ready) (void)hipEventDestroy(c->pend64.ready);
  for (auto &rs : c->slots)
    if (rs.ready) (void)hipEventDestroy(rs.ready);
  if (c->result_done) (void)hipEventDestroy(c->result_done);
  if (c->result_stream) (void)hipStreamDestroy(c->result_stream);
  if (c->lists_final) (void)hipEventDestroy(c->lists_final);
  if (c->peer_read) (void)hipEventDestroy(c->peer_read);
  for (auto *l : {&c->ev_match, &c->ev_prep, &c->ev_merge, &c->ev_proj, &c->ev_pre, &c->ev_rescore})
    for (auto &pr : *l) {
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  for (int b = 0; b < 2; ++b) {
    if (c->stage_filled[b]) (void)hipEventDestroy(c->stage_filled[b]);
    if (c->stage_free[b]) (void)hipEventDestroy(c->stage_free[b]);
    if (c->pending.consumed[b]) (void)hipEventDestroy(c->pending.consumed[b]);
  }
  if (c->pending.filled) (void)hipEventDestroy(c->pending.filled);
  if (c->copy_stream) {
    (void)hipStreamSynchronize(c->copy_stream);
    (void)hipStreamDestroy(c->copy_stream);
  }
  if (c->stream2) {
    (void)hipStreamSynchronize(c->stream2);
    (void)hipStreamDestroy(c->stream2);
    (void)hipEventDestroy(c->ev_fork);
    (void)hipEventDestroy(c->ev_join);
  }
  (void)hipStreamDestroy(c->stream);
  delete c;  // (the device and pinned buffers free themselves)
  return KPDI_OK;
}

int kpdi_synchronize(kpdi_ctx *c) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  int rc = use_device(c);
  if (rc) return rc;
  if (c->have_exp && c->have_problem) {
    rc = flush_pending(c);  // "everything pushed has been swept"
    if (rc) return rc;
  }
  if (c->have_problem) {
    rc = flush_pending(c, true);  // ... and everything handed over to be held is prepared
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->result_stream) HIPCHK(hipStreamSynchronize(c->result_stream));
  return KPDI_OK;
}

int kpdi_set_problem(kpdi_ctx *c, int sy, int sx, const uint8_t *signal_mask, int metric, int compute_dtype,
                     int keep_n) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (sy <= 0 || sx <= 0) return fail(KPDI_EINVAL, "detector shape (%d, %d) must be positive", sy, sx);
  if (metric != KPDI_METRIC_NCC && metric != KPDI_METRIC_NDP) return fail(KPDI_EINVAL, "unknown metric %d", metric);
  if (compute_dtype != KPDI_COMPUTE_F32 && compute_dtype != KPDI_COMPUTE_F16X2 && compute_dtype != KPDI_COMPUTE_F16 &&
      compute_dtype != KPDI_COMPUTE_F64)
    return fail(KPDI_EINVAL, "unknown compute dtype %d", compute_dtype);
  // float64 arithmetic = the f32 path as the screen + rescoring in double (rescore.hip)
  const bool exact64 = compute_dtype == KPDI_COMPUTE_F64;
  if (exact64) compute_dtype = KPDI_COMPUTE_F32;
  if (keep_n <= 0) return fail(KPDI_EINVAL, "keep_n must be >= 1");
  int rc = use_device(c);
  if (rc) return rc;
  c->sw.read();
  const int npix = sy * sx;
  std::vector<int> keep;
  if (signal_mask) {
    for (int i = 0; i < npix; ++i)
      if (!signal_mask[i]) keep.push_back(i);
    if (keep.empty()) return fail(KPDI_EINVAL, "the signal mask excludes every pixel");
    HIPCHK(c->pix_map.reserve(keep.size() * sizeof(int)));
    HIPCHK(hipMemcpyAsync(c->pix_map.p, keep.data(), keep.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    std::vector<unsigned> desc;
    c->have_quad_desc = kpdi::gather_descriptors(keep.data(), (int)keep.size(), npix, &desc);
    if (c->have_quad_desc) {
      HIPCHK(c->quad_desc.reserve(desc.size() * sizeof(unsigned)));
      HIPCHK(hipMemcpyAsync(c->quad_desc.p, desc.data(), desc.size() * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
  } else {
    c->have_quad_desc = false;
  }
  if ((c->pend.st || c->pend.dy) && c->have_exp && (sy != c->sy || sx != c->sx)) {
    bool dummy = false;  // recorded background-removal steps belong to the old detector shape
    rc = flush_preprocess(c, false, &dummy);
    if (rc) return rc;
  }
  if (npix != c->npix) c->have_exp = false;  // resident patterns belong to another detector shape
  // the prepared layout of held chunks depends on shape, mask, metric and arithmetic
  int waves = 8;
  if (const char *e = getenv("KPDI_F16_WAVES")) waves = atoi(e) == 4 ? 4 : 8;
  // the f32 kernel in use (match.hip / the one-wave form of match16.hip) is chosen when the first chunk of a sweep arrives
  // (decide_form); until then - and whenever it cannot change any more - the previous choice stands
  const int wide_mode = getenv("KPDI_F32_WIDE") ? (atoi(getenv("KPDI_F32_WIDE")) != 0) : -1;
  bool wide32 = compute_dtype == KPDI_COMPUTE_F32 && (wide_mode == 1 || (wide_mode < 0 && c->have_problem && c->wide32));
  if (!c->have_problem || sy != c->sy || sx != c->sx || metric != c->metric || compute_dtype != c->compute ||
      (signal_mask != nullptr) != c->have_sig_mask || keep != c->kept_pixels || wide32 != c->wide32)
    release_held(c);
  c->f16_waves = waves;
  c->wide32 = wide32;
  c->wide_mode = wide_mode;
  c->metric = metric;
  c->compute = compute_dtype;
  kpdi::set_detector_layout(c, sy, sx, signal_mask != nullptr, std::move(keep));
  c->exact64 = exact64;
  c->keep_n = keep_n;
  c->have_problem = true;
  c->exp_prepared = false;
  c->run_valid = false;
  discard_pending(c);
  c->final_valid = false;
  return KPDI_OK;
}

int kpdi_set_keep_n(kpdi_ctx *c, int keep_n) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_problem) return fail(KPDI_EINVAL, "kpdi_set_problem has not been called");
  if (keep_n <= 0) return fail(KPDI_EINVAL, "keep_n must be >= 1");
  c->keep_n = keep_n;
  c->run_valid = false;
  discard_pending(c);
  c->final_valid = false;
  return KPDI_OK;
}

int kpdi_set_experimental(kpdi_ctx *c, const void *patterns, int dtype, int64_t m_all, const uint8_t *nav_mask) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  int rc = use_device(c);
  if (rc) return rc;
  return set_experimental_common(c, patterns, false, dtype, m_all, nav_mask);
}

int kpdi_set_experimental_dev(kpdi_ctx *c, const void *d_patterns, int dtype, int64_t m_all,
                              const uint8_t *nav_mask) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  int rc = use_device(c);
  if (rc) return rc;
  return set_experimental_common(c, d_patterns, true, dtype, m_all, nav_mask);
}

int64_t kpdi_n_experimental(kpdi_ctx *c) { return c && c->have_exp ? c->m : 0; }

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
  int rc = use_device(c);
  if (rc) return rc;
  bool dummy = false;
  rc = flush_preprocess(c, false, &dummy);  // recorded background-removal steps run now
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
  const kpdi::IqPlan plan = kpdi::iq_plan(sy, sx, c->m_all);
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
  const kpdi::FfPlan plan = kpdi::ff_plan(freq ? kpdi::FF_DOMAIN_FREQUENCY : kpdi::FF_DOMAIN_SPATIAL, sy, sx, c->m_all);
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
  if (!intensity_dtype(a.dtype_out))
    return fail(KPDI_EINVAL, "dtype_out %d: intensity rescaling writes uint8/int8/uint16/int16/float32/float64", a.dtype_out);
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
  if (!same) {
    std::swap(c->exp_raw, c->int_out);
    c->exp_dtype = a.dtype_out;
  }
  patterns_changed(c);
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
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp) return fail(KPDI_EINVAL, "kpdi_set_experimental has not been called");
  kpdi::IntLaunch a{};
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
  std::swap(c->exp_raw, c->int_out);
  patterns_changed(c);
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
  if (!kpdi::intensity_dtype(dtype_out))
    return fail(KPDI_EINVAL, "dtype_out %d: downsampling writes uint8/int8/uint16/int16/float32/float64", dtype_out);
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
  std::swap(c->exp_raw, c->int_out);
  c->exp_dtype = dtype_out;
  // the problem follows the patterns: the binned detector without a signal mask; metric, arithmetic and keep_n stay
  // (there are no held chunks to release)
  kpdi::set_detector_layout(c, ny, nx, false, {});
  kpdi::patterns_changed(c);
  return KPDI_OK;
}

int kpdi_get_dynamic_background(kpdi_ctx *c, int filter_domain, double std, double truncate, int dtype_out, void *out) {
  int rc = kpdi::check_patterns(c, "the dynamic background");
  if (rc) return rc;
  if (!out) return fail(KPDI_EINVAL, "out is NULL");
  if (!kpdi::intensity_dtype(dtype_out))
    return fail(KPDI_EINVAL, "dtype_out %d: the dynamic background is written as uint8/int8/uint16/int16/float32/float64", dtype_out);
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
  std::swap(c->exp_raw, c->int_out);
  c->exp_dtype = dtype_out;
  kpdi::patterns_changed(c);
  return KPDI_OK;
}

int kpdi_change_dtype(kpdi_ctx *c, int dtype_out) {
  int rc = kpdi::check_patterns(c, "a dtype change");
  if (rc) return rc;
  if (!kpdi::intensity_dtype(dtype_out))
    return fail(KPDI_EINVAL, "dtype_out %d: patterns are cast to uint8/int8/uint16/int16/float32/float64", dtype_out);
  rc = kpdi::start_pattern_op(c);
  if (rc) return rc;
  if (dtype_out == c->exp_dtype) return KPDI_OK;
  const int64_t count = c->m_all * (int64_t)c->npix;
  HIPCHK(c->int_out.reserve((size_t)count * kpdi::dtype_size(dtype_out)));
  hipError_t e = kpdi::launch_change_dtype(c->exp_raw.p, c->exp_dtype, c->int_out.p, dtype_out, count, c->stream);
  if (e != hipSuccess) return fail(KPDI_EHIP, "dtype change kernel: %s (dtype %d -> %d)", hipGetErrorString(e), c->exp_dtype, dtype_out);
  std::swap(c->exp_raw, c->int_out);
  c->exp_dtype = dtype_out;
  kpdi::patterns_changed(c);
  return KPDI_OK;
}

int kpdi_kinematical_master_pattern(kpdi_ctx *c, const double *unit_vectors, const double *theta, const double *intensity,
                                    int64_t m, int half_size, int hemispheres, double *out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!unit_vectors || !theta || !intensity || !out) return fail(KPDI_EINVAL, "unit_vectors, theta, intensity or out is NULL");
  if (m < 1 || m > INT_MAX) return fail(KPDI_EINVAL, "%lld reflectors: at least one is needed", (long long)m);
  if (half_size < 0 || half_size > kpdi::KIN_MAX_HALF_SIZE)
    return fail(KPDI_EINVAL, "half_size %d: between 0 and %d", half_size, kpdi::KIN_MAX_HALF_SIZE);
  if (!kpdi::kin_hemispheres(hemispheres))
    return fail(KPDI_EINVAL, "hemispheres %d: 0 (upper), 1 (lower) or 2 (both)", hemispheres);
  const kpdi::KinPlan plan = kpdi::kinematical_launch_plan(m, half_size, hemispheres);
  if (!plan.ok) return fail(KPDI_EINVAL, "kinematical master pattern of half_size %d from %lld reflectors: no kernel takes this shape",
                            half_size, (long long)m);
  int rc = use_device(c);
  if (rc) return rc;
  // the pixel directions of the upper hemisphere and the reflector table, on the host with NumPy's operations
  const int size = plan.size;
  std::vector<double> axis((size_t)size), dirs((size_t)plan.pixels * 3), table((size_t)m * kpdi::KIN_ENTRY_DOUBLES);
  for (int i = 0; i < size; ++i) axis[(size_t)i] = kpdi::kin_axis(i, size);
  for (int r = 0; r < size; ++r)
    for (int col = 0; col < size; ++col) kpdi::kin_direction(axis[(size_t)col], axis[(size_t)r], &dirs[((size_t)r * size + col) * 3]);
  const double half_pi = 1.5707963267948966;  // np.pi / 2
  for (int64_t i = 0; i < m; ++i) {
    double *e = &table[(size_t)i * kpdi::KIN_ENTRY_DOUBLES];
    e[0] = unit_vectors[3 * i];
    e[1] = unit_vectors[3 * i + 1];
    e[2] = unit_vectors[3 * i + 2];
    e[3] = intensity[i];
    e[6] = half_pi - theta[i];
    kpdi::kin_screen(e[6], &e[4], &e[5]);
    e[7] = 0.0;
  }
  const size_t out_bytes = (size_t)plan.hemispheres * (size_t)plan.pixels * sizeof(double);
  HIPCHK(c->kin_dirs.reserve(dirs.size() * sizeof(double)));
  HIPCHK(c->kin_table.reserve(table.size() * sizeof(double)));
  HIPCHK(c->kin_out.reserve(out_bytes));
  HIPCHK(hipMemcpyAsync(c->kin_dirs.p, dirs.data(), dirs.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->kin_table.p, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  kpdi::KinLaunch l{};
  l.dirs = c->kin_dirs.as<double>();
  l.table = c->kin_table.as<double>();
  l.m = m;
  l.half_size = half_size;
  l.hemispheres = hemispheres;
  l.out = c->kin_out.as<double>();
  kpdi::EventPair timer(c, c->profiling != 0);
  HIPCHK(timer.begin());
  hipError_t e = kpdi::launch_kinematical_master_pattern(l, c->stream);
  (void)timer.end();
  if (e == hipSuccess) rc = kpdi::results_to_host(c, out, c->kin_out.p, out_bytes);  // (synchronises: the host tables are read)
  float ms = 0.f;
  if (e == hipSuccess && rc == KPDI_OK && timer.elapsed(&ms) == hipSuccess) c->cnt.kinematical_ms = ms;
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "kinematical master pattern kernel: %s (half_size %d, %lld reflectors)", hipGetErrorString(e), half_size,
                (long long)m);
  return rc;
}

// the per-point entries of a geometrical simulation, formed on the host (geometrical_plan.h) and uploaded to c->geo_points
static int geometrical_points(kpdi_ctx *c, const double *rotations, int64_t n_points, const double *u_s, const double *a_star,
                              const double *a_direct, const double *pcs, int64_t n_pc) {
  std::vector<double> entries((size_t)n_points * kpdi::GEO_ENTRY_DOUBLES);
  for (int64_t p = 0; p < n_points; ++p)
    kpdi::geo_point_entry(rotations + 4 * p, u_s, a_star, a_direct, pcs + (n_pc == 1 ? 0 : p) * kpdi::GEO_PC_DOUBLES,
                          &entries[(size_t)p * kpdi::GEO_ENTRY_DOUBLES]);
  HIPCHK(c->geo_points.reserve(entries.size() * sizeof(double)));
  HIPCHK(hipMemcpyAsync(c->geo_points.p, entries.data(), entries.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // `entries` leaves scope
  return KPDI_OK;
}

static int geometrical_shape_refused(int64_t n_points, int64_t n_pc) {
  if (n_points < 1 || n_points > INT_MAX) return fail(KPDI_EINVAL, "%lld map points: at least one is needed", (long long)n_points);
  if (n_pc != 1 && n_pc != n_points)
    return fail(KPDI_EINVAL, "%lld projection centres for %lld map points: one, or one per point", (long long)n_pc, (long long)n_points);
  return KPDI_OK;
}

int kpdi_geometrical_visibility(kpdi_ctx *c, const double *vectors, int64_t m, int kind, const double *rotations,
                                int64_t n_points, const double *u_s, const double *basis, const double *pcs, int64_t n_pc,
                                uint8_t *flags) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!vectors || !rotations || !u_s || !basis || !pcs || !flags)
    return fail(KPDI_EINVAL, "vectors, rotations, u_s, basis, pcs or flags is NULL");
  if (m < 1 || m > INT_MAX) return fail(KPDI_EINVAL, "%lld features: at least one is needed", (long long)m);
  int rc = geometrical_shape_refused(n_points, n_pc);
  if (rc) return rc;
  if (kind != KPDI_GEOMETRICAL_LINES && kind != KPDI_GEOMETRICAL_ZONE_AXES)
    return fail(KPDI_EINVAL, "kind %d: 0 (lines) or 1 (zone axes)", kind);
  const kpdi::GeoVisPlan plan = kpdi::geometrical_visibility_plan(m, n_points);
  if (!plan.ok) return fail(KPDI_EINVAL, "visibility of %lld features at %lld map points: no kernel takes this shape", (long long)m,
                            (long long)n_points);
  rc = use_device(c);
  if (rc) return rc;
  rc = geometrical_points(c, rotations, n_points, u_s, kind == KPDI_GEOMETRICAL_LINES ? basis : nullptr,
                          kind == KPDI_GEOMETRICAL_ZONE_AXES ? basis : nullptr, pcs, n_pc);
  if (rc) return rc;
  const size_t vec_bytes = (size_t)m * 3 * sizeof(double), partial_bytes = (size_t)plan.grid_y * (size_t)m;
  HIPCHK(c->geo_vec.reserve(vec_bytes));
  HIPCHK(c->geo_flags.reserve(partial_bytes + (size_t)m));
  HIPCHK(hipMemcpyAsync(c->geo_vec.p, vectors, vec_bytes, hipMemcpyHostToDevice, c->stream));
  kpdi::GeoVisLaunch l{};
  l.vec = c->geo_vec.as<double>();
  l.points = c->geo_points.as<double>();
  l.m = m;
  l.n_points = n_points;
  l.kind = kind;
  l.partial = c->geo_flags.as<uint8_t>();
  l.flags = c->geo_flags.as<uint8_t>() + partial_bytes;
  kpdi::EventPair timer(c, c->profiling != 0);
  HIPCHK(timer.begin());
  hipError_t e = kpdi::launch_geometrical_visibility(l, c->stream);
  (void)timer.end();
  if (e == hipSuccess) rc = kpdi::results_to_host(c, flags, l.flags, (size_t)m);  // (synchronises: `vectors` has been read)
  float ms = 0.f;
  if (e == hipSuccess && rc == KPDI_OK && timer.elapsed(&ms) == hipSuccess) c->cnt.geometrical_visibility_ms = ms;
  if (e != hipSuccess)
    return fail(KPDI_EHIP, "geometrical visibility kernel: %s (%lld features, %lld map points)", hipGetErrorString(e), (long long)m,
                (long long)n_points);
  return rc;
}

int kpdi_geometrical_coordinates(kpdi_ctx *c, const double *hkl, int64_t m, const double *uvw, int64_t z,
                                 const double *rotations, int64_t n_points, const double *u_s, const double *a_star,
                                 const double *a_direct, const double *pcs, int64_t n_pc, double r_gnomonic,
                                 uint8_t *line_in_pattern, double *line_gnomonic, double *line_pixel,
                                 uint8_t *zone_in_pattern, double *zone_gnomonic, double *zone_pixel) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!hkl || !rotations || !u_s || !a_star || !a_direct || !pcs || !line_in_pattern || !line_gnomonic || !line_pixel)
    return fail(KPDI_EINVAL, "hkl, rotations, u_s, a_star, a_direct, pcs or a line output is NULL");
  if (m < 1 || m > INT_MAX) return fail(KPDI_EINVAL, "%lld lines: at least one is needed", (long long)m);
  if (z < 0 || z > INT_MAX) return fail(KPDI_EINVAL, "%lld zone axes: none or more", (long long)z);
  if (z > 0 && (!uvw || !zone_in_pattern || !zone_gnomonic || !zone_pixel))
    return fail(KPDI_EINVAL, "uvw or a zone axis output is NULL");
  int rc = geometrical_shape_refused(n_points, n_pc);
  if (rc) return rc;
  rc = use_device(c);
  if (rc) return rc;
  size_t free_bytes = 0, total_bytes = 0;
  HIPCHK(hipMemGetInfo(&free_bytes, &total_bytes));
  const kpdi::GeoCoordPlan plan = kpdi::geometrical_coord_plan(m, z, n_points, free_bytes / 4);
  if (!plan.ok) return fail(KPDI_EINVAL, "coordinates of %lld lines and %lld zone axes at %lld map points: no kernel takes this shape",
                            (long long)m, (long long)z, (long long)n_points);
  rc = geometrical_points(c, rotations, n_points, u_s, a_star, a_direct, pcs, n_pc);
  if (rc) return rc;
  // the outputs of one pass, each at a multiple of 256 bytes
  const size_t P = (size_t)plan.points, M = (size_t)m, Z = (size_t)z;
  const size_t sizes[6] = {P * M * 4 * sizeof(double), P * M * 4 * sizeof(double), P * Z * 2 * sizeof(double),
                           P * Z * 2 * sizeof(double), P * M, P * Z};
  size_t offset[6], total = 0;
  for (int i = 0; i < 6; ++i) {
    offset[i] = total;
    total += (sizes[i] + 255) / 256 * 256;
  }
  const size_t hkl_bytes = M * 3 * sizeof(double), uvw_bytes = Z * 3 * sizeof(double);
  HIPCHK(c->geo_out.reserve(total));
  HIPCHK(c->geo_vec.reserve((hkl_bytes + 255) / 256 * 256 + uvw_bytes));
  char *vec = c->geo_vec.as<char>(), *out = c->geo_out.as<char>();
  HIPCHK(hipMemcpyAsync(vec, hkl, hkl_bytes, hipMemcpyHostToDevice, c->stream));
  if (z > 0) HIPCHK(hipMemcpyAsync(vec + (hkl_bytes + 255) / 256 * 256, uvw, uvw_bytes, hipMemcpyHostToDevice, c->stream));
  kpdi::EventPair timer(c, c->profiling != 0);  // recorded again in every pass
  double kernel_ms = 0.0;
  hipError_t e = hipSuccess;
  for (int64_t pass = 0; pass < plan.n_passes && e == hipSuccess && rc == KPDI_OK; ++pass) {
    const int64_t p0 = pass * plan.points;
    const size_t np = (size_t)(pass == plan.n_passes - 1 ? plan.tail : plan.points);
    kpdi::GeoCoordLaunch l{};
    l.hkl = reinterpret_cast<const double *>(vec);
    l.uvw = z > 0 ? reinterpret_cast<const double *>(vec + (hkl_bytes + 255) / 256 * 256) : nullptr;
    l.points = c->geo_points.as<double>() + (size_t)p0 * kpdi::GEO_ENTRY_DOUBLES;
    l.m = m;
    l.z = z;
    l.points_in_pass = (int64_t)np;
    l.r_gnomonic = r_gnomonic;
    l.line_gn = reinterpret_cast<double *>(out + offset[0]);
    l.line_px = reinterpret_cast<double *>(out + offset[1]);
    l.zone_gn = z > 0 ? reinterpret_cast<double *>(out + offset[2]) : nullptr;
    l.zone_px = z > 0 ? reinterpret_cast<double *>(out + offset[3]) : nullptr;
    l.line_in = reinterpret_cast<uint8_t *>(out + offset[4]);
    l.zone_in = z > 0 ? reinterpret_cast<uint8_t *>(out + offset[5]) : nullptr;
    (void)timer.begin();
    e = kpdi::launch_geometrical_coordinates(l, c->stream);
    (void)timer.end();
    if (e != hipSuccess) break;
    const size_t at = (size_t)p0;
    rc = kpdi::results_to_host(c, line_gnomonic + at * M * 4, l.line_gn, np * M * 4 * sizeof(double));
    if (rc == KPDI_OK) rc = kpdi::results_to_host(c, line_pixel + at * M * 4, l.line_px, np * M * 4 * sizeof(double));
    if (rc == KPDI_OK) rc = kpdi::results_to_host(c, line_in_pattern + at * M, l.line_in, np * M);
    if (rc == KPDI_OK && z > 0) rc = kpdi::results_to_host(c, zone_gnomonic + at * Z * 2, l.zone_gn, np * Z * 2 * sizeof(double));
    if (rc == KPDI_OK && z > 0) rc = kpdi::results_to_host(c, zone_pixel + at * Z * 2, l.zone_px, np * Z * 2 * sizeof(double));
    if (rc == KPDI_OK && z > 0) rc = kpdi::results_to_host(c, zone_in_pattern + at * Z, l.zone_in, np * Z);
    float ms = 0.f;
    if (rc == KPDI_OK && timer.elapsed(&ms) == hipSuccess) kernel_ms += ms;
  }
  if (timer.on() && e == hipSuccess && rc == KPDI_OK) c->cnt.geometrical_coordinates_ms = kernel_ms;
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);  // the host copies of hkl / uvw may still be in flight
    return fail(KPDI_EHIP, "geometrical coordinates kernel: %s (%lld lines, %lld zone axes, %lld map points)", hipGetErrorString(e),
                (long long)m, (long long)z, (long long)n_points);
  }
  return rc;
}

size_t kpdi_dtype_size(int dtype) { return kpdi::dtype_size(dtype); }

int kpdi_reset_topk(kpdi_ctx *c) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  int rc = use_device(c);
  if (rc) return rc;
  c->run_valid = false;
  discard_pending(c);
  c->final_valid = false;
  return KPDI_OK;
}

int kpdi_dev_alloc(kpdi_ctx *c, size_t bytes, void **d_out) {
  if (!c || !d_out) return fail(KPDI_EINVAL, "NULL argument");
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(hipMalloc(d_out, bytes));
  return KPDI_OK;
}

int kpdi_dev_free(kpdi_ctx *c, void *d_ptr) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipFree(d_ptr));
  return KPDI_OK;
}

int kpdi_h2d(kpdi_ctx *c, void *d_dst, const void *src, size_t bytes) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_d2h(kpdi_ctx *c, void *dst, const void *d_src, size_t bytes) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  int rc = use_device(c);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return KPDI_OK;
}

int kpdi_set_profiling(kpdi_ctx *c, int on) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (on < 0 || on > 3)
    return fail(KPDI_EINVAL, "profiling level %d (0 off, 1 every phase, 2 match launches only, 3 every phase + the epilogue counters)", on);
  c->profiling = on;
  return KPDI_OK;
}

int kpdi_get_counters(kpdi_ctx *c, kpdi_counters *out) {
  if (!c || !out) return fail(KPDI_EINVAL, "NULL argument");
  int rc = use_device(c);
  if (rc) return rc;
  if (c->have_exp && c->have_problem) {
    rc = flush_pending(c);  // (the counters cover everything pushed)
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  rc = drain_events(c, c->ev_match, &c->cnt.match_ms);
  if (rc) return rc;
  rc = drain_events(c, c->ev_prep, &c->cnt.prep_ms);
  if (rc) return rc;
  rc = drain_events(c, c->ev_merge, &c->cnt.merge_ms);
  if (rc) return rc;
  rc = drain_events(c, c->ev_proj, &c->cnt.project_ms);
  if (rc) return rc;
  rc = drain_events(c, c->ev_pre, &c->cnt.preproc_ms);
  if (rc) return rc;
  rc = drain_events(c, c->ev_rescore, &c->cnt.rescore_ms);
  if (rc) return rc;
  rc = drain_events(c, c->ev_comm, &c->cnt.comm_ms);
  if (rc) return rc;
  rc = drain_events(c, c->ev_fixed, &c->cnt.fixed_ms);
  if (rc) return rc;
  if (c->epi_stats.p) {
    unsigned long long st[4];
    HIPCHK(hipMemcpy(st, c->epi_stats.p, sizeof st, hipMemcpyDeviceToHost));
    c->cnt.epi_lists = (int64_t)st[0];
    c->cnt.epi_appended = (int64_t)st[1];
    c->cnt.epi_overflows = (int64_t)st[2];
    c->cnt.epi_direct_first = (int64_t)st[3];
  }
  c->cnt.f64_certificate = c->exact64 ? (c->sw.f64_statistical ? 1 : 2) : 0;
  c->cnt.comm_ranks = 0;
  if (c->comm) {
    int count = 0;
    if (g_rccl.CommCount(c->comm, &count) == ncclSuccess) c->cnt.comm_ranks = count;
  }
  *out = c->cnt;
  return KPDI_OK;
}

int kpdi_reset_counters(kpdi_ctx *c) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  kpdi_counters tmp;
  int rc = kpdi_get_counters(c, &tmp);  // recycles pending events
  if (rc) return rc;
  const int kpad = c->cnt.kpad, kk = c->cnt.k_kept, gr = c->cnt.gather_ranks;
  c->cnt = kpdi_counters{};
  if (c->epi_stats.p) HIPCHK(hipMemsetAsync(c->epi_stats.p, 0, 4 * sizeof(unsigned long long), c->stream));
  c->cnt.kpad = kpad;
  c->cnt.k_kept = kk;
  c->cnt.gather_ranks = gr;
  return KPDI_OK;
}

}  // extern "C"
