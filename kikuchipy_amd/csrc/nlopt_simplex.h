// nlopt_simplex.h - the Nelder-Mead simplex search that NLopt offers as LN_NELDERMEAD, in f64 for the host
// and the device (plain C++17, no HIP headers).  NLopt itself (its nldrmd.c and the front end of
// nlopt_optimize) was NOT available when this was written: the contract is the operation-by-operation text
// of DESIGN.md section 21, and what is pinned is that this header, the device kernels that instantiate it
// and the plain-Python restatement of that text (tests/_nlopt_simplex_restate.py) agree bit for bit
// (tests/test_host_nlopt_simplex.py, tests/test_gpu_nlopt_simplex.py).  Agreement with an installed NLopt
// is NOT checked here (tools/compare_nlopt.py reports it where `import nlopt` works).
//
// Every sum, product and comparison is written in the order and form of that text (a comparison with a NaN
// takes the branch the text gives it), and the file must be compiled WITHOUT fused multiply-add
// (-ffp-contract=off).
//
//   front end   x0 outside [lower, upper] -> INVALID_ARGS, nothing evaluated; variables with
//               lower == upper are held there and leave the simplex; the default initial step
//   CHECK       after every evaluation: ++nevals; f < minf keeps the point; maxeval ends the search
//   start       x0, then x0 with one coordinate stepped (kept inside the box); a step that does not move
//               the coordinate -> FAILURE
//   loop        ftol test, centroid, reflection, then expansion | accept | contraction (| shrink); a
//               reflected point that coincides with the centre or with the point it came from -> XTOL_REACHED
// Ties in f: the LOW point is the one with the lower storage index, the HIGH point the one with the higher;
// the second-highest value is searched among the points other than the high one.
// The centroid is summed from 0.0 over the points other than the high one, in storage order, and multiplied
// once by 1.0 / n.
//
// Termination: a search with ftol_rel <= 0 and no maxeval ends only when the simplex has collapsed (XTOL_REACHED);
// the callers on the device refuse that combination and non-finite starting points.
//
// KPDI_NLOPT_COUNT (host tests only): every named arm increments one entry of `kpdi_nlopt_count`.
#pragma once

#include <cmath>

#ifndef KPDI_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define KPDI_HD __host__ __device__
#else
#define KPDI_HD
#endif
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// clang-format off
#define KPDI_NLOPT_BRANCHES(X)                                                                     \
  X(fe_invalid) X(fe_held) X(fe_free) X(fe_all_held)                                               \
  X(step_given) X(step_range) X(step_upper) X(step_lower) X(step_from_x) X(step_one)               \
  X(chk_better) X(chk_not_better) X(chk_maxeval)                                                   \
  X(st_plain) X(st_above_far) X(st_above_near) X(st_below_far) X(st_below_near)                    \
  X(st_reversed_outside) X(st_no_move)                                                             \
  X(tie_low) X(tie_high)                                                                           \
  X(ftol_relative) X(ftol_equal) X(ftol_not_finite) X(ftol_go_on)                                  \
  X(clamp_lower) X(clamp_upper) X(rf_coincides) X(rf_ok)                              \
  X(expand) X(expand_kept) X(expand_rejected) X(accept_reflection)                                 \
  X(contract_inside) X(contract_outside) X(contract_kept) X(shrink)
// clang-format on

namespace kpdi {

enum NloptBranch {
#define KPDI_NS_ENUM(name) NSB_##name,
  KPDI_NLOPT_BRANCHES(KPDI_NS_ENUM)
#undef KPDI_NS_ENUM
      NSB_COUNT
};

#ifdef KPDI_NLOPT_COUNT
inline long long kpdi_nlopt_count[NSB_COUNT] = {};
inline const char *const kpdi_nlopt_branch_names[NSB_COUNT] = {
#define KPDI_NS_NAME(name) #name,
    KPDI_NLOPT_BRANCHES(KPDI_NS_NAME)
#undef KPDI_NS_NAME
};
#define KPDI_NS_HIT(name) (++::kpdi::kpdi_nlopt_count[::kpdi::NSB_##name])
#else
#define KPDI_NS_HIT(name) ((void)0)
#endif

// NLopt's result codes (nlopt.h)
enum NloptStatus {
  NLOPT_ST_FAILURE = -1,
  NLOPT_ST_INVALID_ARGS = -2,
  NLOPT_ST_SUCCESS = 1,
  NLOPT_ST_FTOL_REACHED = 3,
  NLOPT_ST_XTOL_REACHED = 4,
  NLOPT_ST_MAXEVAL_REACHED = 5,
};

KPDI_HD inline bool ns_close(double a, double b) { return std::fabs(a - b) <= 1e-13 * (std::fabs(a) + std::fabs(b)); }
KPDI_HD inline bool ns_tiny(double v) { return v == 0.0 || std::fabs(v) < 2.2250738585072014e-308; }
KPDI_HD inline bool ns_isinf(double v) { return v == HUGE_VAL || v == -HUGE_VAL; }
KPDI_HD inline bool ns_isfinite(double v) { return (v - v) == 0.0; }

// E: `double eval(const double *x)`, the objective at ALL nvar variables.
template <int NMAX, class E>
struct NloptSimplex {
  E &ev;
  int nvar, n;  // all variables; the free ones (lower != upper), which span the simplex
  int var[NMAX];                        // free variable -> variable
  double lb[NMAX], ub[NMAX], step[NMAX];  // of the free variables
  double pts[NMAX + 1][NMAX], fv[NMAX + 1];
  double c[NMAX], xr[NMAX];
  double xfull[NMAX];  // the point being evaluated, held variables included
  double ftol_rel;
  long long maxeval;
  // results
  int status;
  long long nevals;
  double minf;
  double x[NMAX];  // the best point seen

  KPDI_HD explicit NloptSimplex(E &e) : ev(e) {}

  // CHECK; false = the search ends here
  KPDI_HD bool check(double f) {
    ++nevals;
    if (f < minf) {
      KPDI_NS_HIT(chk_better);
      minf = f;
      for (int i = 0; i < nvar; ++i) x[i] = xfull[i];
    } else {
      KPDI_NS_HIT(chk_not_better);
    }
    if (maxeval > 0 && nevals >= maxeval) {
      KPDI_NS_HIT(chk_maxeval);
      status = NLOPT_ST_MAXEVAL_REACHED;
      return false;
    }
    return true;
  }
  // the objective at free-variable point p, then CHECK
  KPDI_HD bool eval_check(const double *p, double *f) {
    for (int k = 0; k < n; ++k) xfull[var[k]] = p[k];
    *f = ev.eval(xfull);
    return check(*f);
  }

  // dst = centre + scale * (centre - xold), clamped (lower first); false = dst coincides with the centre or with xold.
  // dst may be xold.
  KPDI_HD bool reflect(double *dst, const double *centre, double scale, const double *xold) {
    bool at_centre = true, at_old = true;
    for (int i = 0; i < n; ++i) {
      const double old = xold[i];
      double v = centre[i] + scale * (centre[i] - old);
      if (v < lb[i]) {
        KPDI_NS_HIT(clamp_lower);
        v = lb[i];
      }
      if (v > ub[i]) {
        KPDI_NS_HIT(clamp_upper);
        v = ub[i];
      }
      at_centre = at_centre && ns_close(v, centre[i]);
      at_old = at_old && ns_close(v, old);
      dst[i] = v;
    }
    if (at_centre || at_old) {
      KPDI_NS_HIT(rf_coincides);
      return false;
    }
    KPDI_NS_HIT(rf_ok);
    return true;
  }

  KPDI_HD double default_step(double lo, double hi, double at) {
    double s = HUGE_VAL;
    if (!ns_isinf(hi) && !ns_isinf(lo) && hi > lo && (hi - lo) * 0.25 < s) {
      KPDI_NS_HIT(step_range);
      s = (hi - lo) * 0.25;
    }
    if (!ns_isinf(hi) && hi > at && hi - at < s) {
      KPDI_NS_HIT(step_upper);
      s = (hi - at) * 0.75;
    }
    if (!ns_isinf(lo) && at > lo && at - lo < s) {
      KPDI_NS_HIT(step_lower);
      s = (at - lo) * 0.75;
    }
    if (ns_isinf(s) || ns_tiny(s)) {
      KPDI_NS_HIT(step_from_x);
      s = at;
    }
    if (ns_isinf(s) || ns_tiny(s)) {
      KPDI_NS_HIT(step_one);
      s = 1.0;
    }
    return s;
  }

  // lower / upper / xstep: each null or one value per variable.  max_eval <= 0: no limit.
  // Leaves status, nevals, minf, x.
  KPDI_HD void optimize(int n_variables, const double *x0, const double *lower, const double *upper, const double *xstep,
                        double f_tol_rel, long long max_eval) {
    nvar = n_variables;
    ftol_rel = f_tol_rel;
    maxeval = max_eval;
    nevals = 0;
    minf = HUGE_VAL;
    status = NLOPT_ST_SUCCESS;
    for (int i = 0; i < nvar; ++i) x[i] = xfull[i] = x0[i];

    // ---- front end
    for (int i = 0; i < nvar; ++i) {
      const double lo = lower ? lower[i] : -HUGE_VAL, hi = upper ? upper[i] : HUGE_VAL;
      if (x0[i] < lo || x0[i] > hi) {
        KPDI_NS_HIT(fe_invalid);
        status = NLOPT_ST_INVALID_ARGS;
        return;
      }
    }
    n = 0;
    for (int i = 0; i < nvar; ++i) {
      const double lo = lower ? lower[i] : -HUGE_VAL, hi = upper ? upper[i] : HUGE_VAL;
      if (lo == hi) {
        KPDI_NS_HIT(fe_held);
        x[i] = xfull[i] = lo;
        continue;
      }
      KPDI_NS_HIT(fe_free);
      var[n] = i;
      lb[n] = lo;
      ub[n] = hi;
      if (xstep) {
        KPDI_NS_HIT(step_given);
        step[n] = xstep[i];
      } else {
        step[n] = default_step(lo, hi, x0[i]);
      }
      ++n;
    }
    if (n == 0) {
      KPDI_NS_HIT(fe_all_held);
      minf = ev.eval(xfull);
      nevals = 1;
      return;
    }

    // ---- start
    for (int k = 0; k < n; ++k) pts[0][k] = x0[var[k]];
    fv[0] = ev.eval(xfull);
    minf = fv[0];
    if (!check(fv[0])) return;
    for (int k = 0; k < n; ++k) {
      for (int j = 0; j < n; ++j) pts[k + 1][j] = pts[0][j];
      const double at = pts[0][k], mag = std::fabs(step[k]);
      double p = at + step[k];
      if (p > ub[k]) {
        if (ub[k] - at > mag * 0.1) {
          KPDI_NS_HIT(st_above_far);
          p = ub[k];
        } else {
          KPDI_NS_HIT(st_above_near);
          p = at - mag;
        }
      } else {
        KPDI_NS_HIT(st_plain);
      }
      if (p < lb[k]) {
        if (at - lb[k] > mag * 0.1) {
          KPDI_NS_HIT(st_below_far);
          p = lb[k];
        } else {
          KPDI_NS_HIT(st_below_near);
          p = at + mag;
          if (p > ub[k]) {
            KPDI_NS_HIT(st_reversed_outside);
            p = 0.5 * ((ub[k] - at > at - lb[k] ? ub[k] : lb[k]) + at);
          }
        }
      }
      if (ns_close(p, at)) {
        KPDI_NS_HIT(st_no_move);
        status = NLOPT_ST_FAILURE;
        return;
      }
      pts[k + 1][k] = p;
      if (!eval_check(pts[k + 1], &fv[k + 1])) return;
    }

    // ---- loop
    const double alpha = 1.0, beta = 0.5, gamm = 2.0, delta = 0.5;
    for (;;) {
      int l = 0, h = 0;
      for (int a = 1; a <= n; ++a) {
        if (fv[a] < fv[l]) l = a;    // a tie leaves the lower storage index
        if (fv[a] >= fv[h]) h = a;   // a tie hands over to the higher storage index
      }
      int s = h == 0 ? 1 : 0;  // the highest of the others, by the rule of `h`
      for (int a = s + 1; a <= n; ++a)
        if (a != h && fv[a] >= fv[s]) s = a;
      const double fl = fv[l], fh = fv[h], fs = fv[s];
#ifdef KPDI_NLOPT_COUNT
      {
        bool low = false, high = false;
        for (int a = 0; a <= n; ++a) {
          low = low || (a != l && fv[a] == fl);
          high = high || (a != h && fv[a] == fh);
        }
        if (low) KPDI_NS_HIT(tie_low);
        if (high) KPDI_NS_HIT(tie_high);
      }
#endif

      // 1. ftol
      if (ns_isfinite(fh)) {
        if (std::fabs(fl - fh) < ftol_rel * (std::fabs(fl) + std::fabs(fh)) * 0.5) {
          KPDI_NS_HIT(ftol_relative);
          status = NLOPT_ST_FTOL_REACHED;
          return;
        }
        if (ftol_rel > 0.0 && fl == fh) {
          KPDI_NS_HIT(ftol_equal);
          status = NLOPT_ST_FTOL_REACHED;
          return;
        }
        KPDI_NS_HIT(ftol_go_on);
      } else {
        KPDI_NS_HIT(ftol_not_finite);
      }

      // 2. centroid of the points other than the high one
      for (int i = 0; i < n; ++i) c[i] = 0.0;
      for (int a = 0; a <= n; ++a)
        if (a != h)
          for (int i = 0; i < n; ++i) c[i] += pts[a][i];
      const double inv = 1.0 / (double)n;
      for (int i = 0; i < n; ++i) c[i] *= inv;

      // 3, 4. reflection
      double fr;
      if (!reflect(xr, c, alpha, pts[h])) {
        status = NLOPT_ST_XTOL_REACHED;
        return;
      }
      if (!eval_check(xr, &fr)) return;

      if (fr < fl) {  // 5. expansion, written over the high point
        KPDI_NS_HIT(expand);
        if (!reflect(pts[h], c, gamm, pts[h])) {
          status = NLOPT_ST_XTOL_REACHED;
          return;
        }
        if (!eval_check(pts[h], &fv[h])) return;
        if (fv[h] >= fr) {
          KPDI_NS_HIT(expand_rejected);
          for (int i = 0; i < n; ++i) pts[h][i] = xr[i];
          fv[h] = fr;
        } else {
          KPDI_NS_HIT(expand_kept);
        }
      } else if (fr < fs) {  // 6.
        KPDI_NS_HIT(accept_reflection);
        for (int i = 0; i < n; ++i) pts[h][i] = xr[i];
        fv[h] = fr;
      } else {  // 7. contraction, else shrink towards the low point
        double scale;
        if (fh <= fr) {
          KPDI_NS_HIT(contract_inside);
          scale = -beta;
        } else {
          KPDI_NS_HIT(contract_outside);
          scale = beta;
        }
        double xc[NMAX], fc;
        if (!reflect(xc, c, scale, pts[h])) {
          status = NLOPT_ST_XTOL_REACHED;
          return;
        }
        if (!eval_check(xc, &fc)) return;
        if (fc < fr && fc < fh) {
          KPDI_NS_HIT(contract_kept);
          for (int i = 0; i < n; ++i) pts[h][i] = xc[i];
          fv[h] = fc;
        } else {
          KPDI_NS_HIT(shrink);
          for (int a = 0; a <= n; ++a) {
            if (a == l) continue;
            if (!reflect(pts[a], pts[l], -delta, pts[a])) {
              status = NLOPT_ST_XTOL_REACHED;
              return;
            }
            if (!eval_check(pts[a], &fv[a])) return;
          }
        }
      }
    }
  }
};

}  // namespace kpdi
