// exact64.hip - float64 arithmetic (KPDI_COMPUTE_F64; the reference's `dtype=float64`, _similarity_metric.py:244-253):
// the f32 path screens, rescore.hip rescores the screened candidates in double from the raw patterns and keeps the best-k
// in double; certification of the screen; the float64 hand-over.
// (one of the host translation units api.hip was split into in round 5: context.h holds what they share)
#include "context.h"

using namespace kpdi;

namespace kpdi {

// float64 arithmetic (rescore.hip): screen keep_n + 12 candidates of the chunk in f32, rescore them in double from
// the raw patterns, merge into the running float64 best-k, certify; uncertified patterns get up to EXTRA64 more
// screening passes of 32 candidates
constexpr int MARGIN64 = 12, EXTRA64 = 3;

// screening passes of the pending chunk up to `target` candidates per pattern (each: f32 match + rescoring in double +
// merge into the running float64 best-k with its certification), then the read-back of the last merge's verdict
static int exact64_passes(kpdi_ctx *c, int64_t target) {
  kpdi_ctx::Pending64 &q = c->pend64;
  const int k = c->keep_n;
  const int pass = pass_entries(c);
  const int64_t n_chunk = q.plan.req.n_chunk;
  unsigned *cert = c->cert64.as<unsigned>();
  while (q.done < target) {
    const int kp = (int)std::min<int64_t>(q.done == 0 ? kpdi::KMAX_LIMIT : pass, target - q.done);
    int rc = local_pass(c, q.y, q.plan, q.global_start, q.done, kp, q.cap);
    if (rc) return rc;
    ScopedTimer t(c, &c->ev_rescore);
    kpdi::RescoreLaunch r{};
    r.exp_raw = c->exp_raw.p;
    r.exp_dtype = c->exp_dtype;
    r.row_map = c->have_nav_mask ? c->row_map.as<int>() : nullptr;
    r.dict_raw = q.raw;
    r.dict_dtype = q.raw_dtype;
    r.n_chunk = n_chunk;
    r.global_start = q.global_start;
    r.pix_map = c->have_sig_mask ? c->pix_map.as<int>() : nullptr;
    r.k = c->k_kept;
    r.npix = c->npix;
    r.metric = c->metric;
    r.m = c->m;
    r.cand_s = c->loc_s.as<float>();
    r.cand_i = c->loc_i.as<int>();
    r.cand_stride = q.cap;
    r.cand_offset = q.done;
    r.n_cand = kp;
    r.cand_s64 = c->cand64.as<double>();
    r.max_diff = cert;
    r.exp_degenerate = c->xdeg64.as<int>();
    HIPCHK(kpdi::launch_rescore(r, c->stream));
    HIPCHK(hipMemsetAsync(cert + 1, 0, sizeof(unsigned), c->stream));
    kpdi::Merge64Launch g{};
    g.m = c->m;
    g.k = k;
    g.run_s = c->run64_s.as<double>();
    g.run_i = c->run64_i.as<int>();
    g.cand_s64 = c->cand64.as<double>() + q.done;
    g.cand_i = c->loc_i.as<int>() + q.done;
    g.lists = 1;
    g.len = kp;
    g.row_stride = q.cap;
    g.list_stride = 0;
    g.out_s = c->run64_s.as<double>();
    g.out_i = c->run64_i.as<int>();
    g.cand_s32 = c->loc_s.as<float>();
    g.s32_stride = q.cap;
    g.s32_col = q.done + kp - 1;
    g.enumerated_all = q.done + kp >= n_chunk;
    g.max_diff = cert;
    // what an unscreened candidate's float64 score may exceed its float32 score by: at least the worst-case
    // accumulation bound of a K-term float32 dot product of unit vectors, (K + 2) 2^-24 (2.1e-4 at K = 3600) - a
    // certificate that holds for ANY data (the default since round 5: the gap between the keep_n-th and the last
    // screened score of ordinary data is ~2.5e-3, so the proof costs no extra pass there; tools/f64_probe.py measures
    // the adversarial near-tie set).  KPDI_F64_EPS=statistical: round 4's default - 8 x the largest difference seen
    // among the rescored pairs of the sweep (~130 000 samples per chunk at configs[1], taken from the best-scoring
    // pairs, whose partial sums - and rounding errors - are the largest), never less than 1e-6: fewer screening passes
    // where the k-th and the screened-last scores are closer than the worst case, no proof.
    g.eps_floor = c->sw.f64_statistical ? 1e-6f : (float)((c->k_kept + 2) * 0x1p-24 * 1.01) + 1e-6f;
    g.uncertified = (int *)(cert + 1);
    g.exp_degenerate = c->xdeg64.as<int>();
    HIPCHK(kpdi::launch_merge64(g, c->stream));
    q.done += kp;
  }
  HIPCHK(hipMemcpyAsync(q.flag.p, cert + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipEventRecord(q.ready, c->stream));
  return KPDI_OK;
}

// Look at the pending chunk's verdict; patterns it left uncertified get up to EXTRA64 more screening passes of the SAME
// chunk - whose prepared form, raw patterns and candidate buffers are still in place: every entry point comes through
// here (use_device) before it touches them.
int resolve_exact64(kpdi_ctx *c) {
  kpdi_ctx::Pending64 &q = c->pend64;
  if (!q.active) return KPDI_OK;
  const int64_t n_chunk = q.plan.req.n_chunk;
  q.active = false;  // (an error below leaves no half-resolved chunk behind)
  bool more = false;
  int uncertified = 0;
  for (;;) {
    HIPCHK(hipEventSynchronize(q.ready));
    uncertified = *(volatile int *)q.flag.p;
    if (uncertified == 0 || q.done >= n_chunk || q.extra == EXTRA64) break;
    ++q.extra;
    c->cnt.rescore_extra_passes += 1;
    more = true;
    int rc = exact64_passes(c, std::min<int64_t>((int64_t)q.done + pass_entries(c), n_chunk));
    if (rc) return rc;
  }
  c->cnt.uncertified_patterns += uncertified;
  // the extra passes read the chunk's staging buffer after staged_upload released it: release both again, behind them
  if (more && c->copy_stream)
    for (int b = 0; b < 2; ++b) HIPCHK(hipEventRecord(c->stage_free[b], c->stream));
  return KPDI_OK;
}

// float64 arithmetic (rescore.hip): screen keep_n + 12 candidates of the chunk in f32, rescore them in double from
// the raw patterns, merge into the running float64 best-k, certify; uncertified patterns get up to EXTRA64 more
// screening passes of 32 candidates.  The verdict of the first passes is read back asynchronously: a caller streaming
// host chunks (kpdi_push_dictionary_chunk) looks at it only after the NEXT chunk's upload has been queued, so that
// upload and sweep overlap as they do in the float32 modes; everyone else resolves it before returning.
int sweep_exact64(kpdi_ctx *c, const float *y, const plan::SweepPlan &chunk, int64_t global_start, const void *raw, int raw_dtype) {
  const int k = c->keep_n;
  const int64_t n_chunk = chunk.req.n_chunk;
  if ((int64_t)k + MARGIN64 > 4096) return fail(KPDI_EINVAL, "float64 arithmetic supports keep_n <= %d", 4096 - MARGIN64);
  const int pass = pass_entries(c);
  const int cap = kpdi::round_up(k + MARGIN64, pass) + pass * EXTRA64;
  const size_t n = (size_t)c->m * cap;
  HIPCHK(c->loc_s.reserve(n * sizeof(float)));
  HIPCHK(c->loc_i.reserve(n * sizeof(int)));
  HIPCHK(c->cand64.reserve(n * sizeof(double)));
  HIPCHK(c->xdeg64.reserve((size_t)std::max(c->m, 1) * sizeof(int)));
  HIPCHK(c->bound_s.reserve((size_t)c->m_pad * sizeof(float)));
  HIPCHK(c->bound_i.reserve((size_t)c->m_pad * sizeof(int)));
  HIPCHK(kpdi::launch_fill_topk(c->bound_s.as<float>(), c->bound_i.as<int>(), c->m_pad, c->stream));
  HIPCHK(kpdi::launch_fill_topk(c->loc_s.as<float>(), c->loc_i.as<int>(), (int64_t)n, c->stream));
  kpdi_ctx::Pending64 &q = c->pend64;
  HIPCHK(q.ready.ensure());
  HIPCHK(q.flag.reserve(sizeof(int)));
  q.y = y;
  q.raw = raw;
  q.raw_dtype = raw_dtype;
  q.plan = chunk;
  q.cap = cap;
  q.done = 0;
  q.extra = 0;
  q.global_start = global_start;
  int rc = exact64_passes(c, std::min<int64_t>((int64_t)k + MARGIN64, n_chunk));
  if (rc) return rc;
  q.active = true;
  return q.defer && !c->sw.f64_sync ? KPDI_OK : resolve_exact64(c);  // (KPDI_F64_SYNC: round 2's behaviour, A/B)
}

// float64 arithmetic: the running double lists (all-gathered and merged over the ranks) to the host;
// exactly one of scores64 / scores32 is set
int finalize64(kpdi_ctx *c, double *scores64, float *scores32, int64_t *indices_out) {
  const int k = c->keep_n;
  const size_t n = (size_t)c->m * k;
  const double *d_s = c->run64_s.as<double>();
  const int *d_i = c->run64_i.as<int>();
  // the lists of all ranks: RCCL all-gather (one process per GPU, or an in-process communicator), or - members of an
  // in-process group with peer-copy gather - already copied into the gather buffers by kpdi::root_gather_p2p
  const int ranks = c->p2p_ranks ? c->p2p_ranks : (c->comm ? c->nranks : 0);
  const bool peer_copied = c->p2p_ranks > 0;
  c->p2p_ranks = 0;
  c->cnt.gather_ranks = ranks;
  if (ranks) {
    HIPCHK(c->final64_s.reserve(n * sizeof(double)));
    HIPCHK(c->final64_i.reserve(n * sizeof(int)));
    if (!peer_copied) {
      HIPCHK(c->gather64_s.reserve(n * ranks * sizeof(double)));
      HIPCHK(c->gather64_i.reserve(n * ranks * sizeof(int)));
      ncclResult_t r;
      {
        ScopedTimer t(c, &c->ev_comm);
        r = g_rccl.GroupStart();
        if (r == ncclSuccess) r = g_rccl.AllGather(d_s, c->gather64_s.p, n, ncclFloat64, c->comm, c->stream);
        if (r == ncclSuccess) r = g_rccl.AllGather(d_i, c->gather64_i.p, n, ncclInt32, c->comm, c->stream);
        ncclResult_t r2 = g_rccl.GroupEnd();
        if (r == ncclSuccess) r = r2;
      }
      if (r != ncclSuccess) return fail(KPDI_ECOMM, "RCCL all-gather failed: %s", g_rccl.GetErrorString(r));
    }
    // merge64_kernel ranks a pattern's candidates in LDS (12 bytes each): the per-rank lists join in groups that fit -
    // all at once for ordinary keep_n, a few ranks at a time for very long lists (8 ranks x keep_n > 1600 exceeded the
    // LDS of one launch and used to fail here, after the whole sweep, with a bare HIP error)
    const size_t lds_entries = (150 * 1024) / (sizeof(double) + sizeof(int));
    if ((size_t)2 * k > lds_entries)
      return fail(KPDI_EINVAL, "keep_n = %d is too large for the float64 merge of several ranks (limit %zu)", k, lds_entries / 2);
    {
      ScopedTimer t(c, &c->ev_merge);
      for (int r0 = 0; r0 < ranks;) {
        const size_t room = lds_entries - (r0 ? (size_t)k : 0);
        const int group = (int)std::min<size_t>(ranks - r0, std::max<size_t>(room / k, 1));
        kpdi::Merge64Launch g{};
        g.m = c->m;
        g.k = k;
        g.run_s = r0 ? c->final64_s.as<double>() : nullptr;  // the result so far (in place: read into LDS first)
        g.run_i = r0 ? c->final64_i.as<int>() : nullptr;
        g.cand_s64 = c->gather64_s.as<double>() + (size_t)r0 * n;
        g.cand_i = c->gather64_i.as<int>() + (size_t)r0 * n;
        g.lists = group;
        g.len = k;
        g.row_stride = k;
        g.list_stride = (int64_t)n;
        g.out_s = c->final64_s.as<double>();
        g.out_i = c->final64_i.as<int>();
        HIPCHK(kpdi::launch_merge64(g, c->stream));
        r0 += group;
      }
    }
    d_s = c->final64_s.as<double>();
    d_i = c->final64_i.as<int>();
  }
  c->final_idx = d_i;
  c->final_valid = true;
  if (!indices_out) return KPDI_OK;  // a group member that only takes part in the all-gather (kpdi::finalize_participate)
  // through the page-locked staging buffer of kpdi_finalize (a copy into pageable memory is pinned on the fly by the
  // runtime: milliseconds, and slower kernels behind it)
  std::vector<double> hs_pageable;
  std::vector<int> hi_pageable;
  double *hs;
  int *hi;
  if (c->pin_out.reserve(n * (sizeof(double) + sizeof(int))) == hipSuccess) {
    hs = (double *)c->pin_out.p;
    hi = (int *)(hs + n);
  } else {
    (void)hipGetLastError();
    hs_pageable.resize(n);
    hi_pageable.resize(n);
    hs = hs_pageable.data();
    hi = hi_pageable.data();
  }
  c->result_i32 = nullptr;
  HIPCHK(hipMemcpyAsync(hs, d_s, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hi, d_i, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n; ++i) {
    if (scores64) scores64[i] = hs[i];
    if (scores32) scores32[i] = (float)hs[i];
    indices_out[i] = (int64_t)hi[i];
  }
  return KPDI_OK;
}

}  // namespace kpdi

extern "C" {

int kpdi_finalize_f64(kpdi_ctx *c, double *scores_out, int64_t *indices_out) {
  if (!c) return fail(KPDI_EINVAL, "ctx is NULL");
  if (!c->have_exp || !c->have_problem) return fail(KPDI_EINVAL, "nothing to finalise");
  if (!scores_out || !indices_out) return fail(KPDI_EINVAL, "output pointer is NULL");
  if (!c->exact64) return fail(KPDI_EINVAL, "kpdi_finalize_f64 needs a problem set up with KPDI_COMPUTE_F64");
  int rc = use_device(c);
  if (rc) return rc;
  if (c->m == 0) return KPDI_OK;
  rc = ensure_running(c);  // a rank that pushed nothing contributes empty lists
  if (rc) return rc;
  return finalize64(c, scores_out, nullptr, indices_out);
}

}  // extern "C"
