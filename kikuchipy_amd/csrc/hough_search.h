// hough_search.h - the projection-centre search of one pattern (EBSD.hough_indexing_optimize_pc with batch=True; DESIGN.md
// section 28): the objective of kikuchipy_amd/indexing/_hough_indexing.py for one pattern and SciPy's Nelder-Mead
// (nelder_mead.h) around it, as a search that is advanced a bounded number of evaluations at a time.  Pure functions:
// `__host__ __device__` under hipcc, plain inline functions under a host compiler (tests/test_host_hough_pc_search.py
// compiles this header); float64; compile WITHOUT fused multiply-add (-ffp-contract=off), like hough_vote.h.
//
// The objective at a projection centre pc, over the detected bands of the pattern:
//   pc[2] > 0 is false                 -> 180
//   n_valid = bands with valid != 0 (NOT the bands whose normal is finite: the host path counts the records)
//   (fit, nmatch) = hv_index of the finite normals of the valid bands under pc (nmatch = 0 when not indexed)
//   charged = (nmatch > 0 ? fit nmatch : 0) + tol_deg (n_valid - nmatch)
//   n_valid > 0 ? charged / n_valid : tol_deg
// every operation in the order the host path writes it, so that both return the same bits.
#pragma once
#include "hough_plan.h"
#include "hough_vote.h"
#include "nelder_mead.h"

namespace kpdi {

// what every search of one call shares
struct HoughPcSearchOptions {
  double pc0[3];
  double xatol, fatol;
  int maxiter, maxfun;  // resolved: both >= 1 (`resolve_budget`)
  double tol_deg;       // the tolerance of the vote in degrees, what an unmatched band is charged
};

// one pattern's search between two launches; all zero = not begun
struct HoughPcSearch {
  NelderMead<3> nm;
  int32_t begun;
};

HV_HD double hv_pc_objective(const HoughBand *bands, int n_bands, const double *pc, const HvDetector &det, const HvPhase &ph,
                             double tol_deg) {
  if (!(pc[2] > 0.0)) return 180.0;
  double normals[HV_MAX_BANDS][3];
  int nb = 0, n_valid = 0;
  for (int b = 0; b < n_bands; ++b) {
    if (!bands[b].valid) continue;
    ++n_valid;
    if (hv_band_normal((double)bands[b].theta, (double)bands[b].rho, pc, det.ny, det.nx, normals[nb])) ++nb;
  }
  const HvResult r = hv_index(normals, nb, n_bands, ph, det);
  const int nmatch = r.indexed ? r.nmatch : 0;
  const double charged = (nmatch > 0 ? r.fit * (double)nmatch : 0.0) + tol_deg * (double)(n_valid - nmatch);
  return n_valid > 0 ? charged / (double)n_valid : tol_deg;
}

HV_HD bool hv_pc_search_done(const HoughPcSearch &s) { return s.begun && s.nm.state == NelderMead<3>::S_DONE; }

// advances the search by at most `max_evals` evaluations of the objective (the first call begins it from o.pc0) and
// returns whether it is done.  A bounded loop whose body every search walks alike: a search that is done idles through
// it, so the lanes of a wave reach the vote together.
HV_HD bool hv_pc_search_advance(HoughPcSearch &s, const HoughBand *bands, int n_bands, const HvDetector &det, const HvPhase &ph,
                                const HoughPcSearchOptions &o, int max_evals) {
  if (!s.begun) {
    s.nm.begin(3, o.pc0, nullptr, nullptr, o.xatol, o.fatol, o.maxiter, o.maxfun);
    s.begun = 1;
  }
  for (int e = 0; e < max_evals; ++e) {
    const bool live = s.nm.state != NelderMead<3>::S_DONE;
    double f = 0.0;
    if (live) f = hv_pc_objective(bands, n_bands, s.nm.xeval, det, ph, o.tol_deg);
    if (live) s.nm.feed(f);
  }
  return s.nm.state == NelderMead<3>::S_DONE;
}

// SciPy's OptimizeResult.status of a finished search: 1 the evaluations ran out, 2 the iterations did, 0 converged
HV_HD int hv_pc_search_status(const HoughPcSearch &s) {
  return s.nm.fcalls >= s.nm.maxfun ? 1 : (s.nm.iterations >= s.nm.maxiter ? 2 : 0);
}

// what one launch of the search kernel takes (device pointers)
struct HoughPcSearchLaunch {
  const HoughBand *bands;  // [m][n_bands]
  int64_t m;
  int n_bands;
  HvDetector det;
  HvPhase phase;
  HoughPcSearchOptions options;
  int evals;               // evaluations per lane in this launch, >= 1
  HoughPcSearch *states;   // [m], zeroed before the first launch
  uint8_t *done;           // [m]
};

}  // namespace kpdi
