// powell.h - scipy.optimize.minimize(method="Powell") of SciPy 1.15.3, restated operation for
// operation in f64 for the host and the device (plain C++17, no HIP headers).
//   scipy/optimize/_optimize.py
//     :530-554    _wrap_scalar_function_maxfun_validation   -> Powell::call
//     :2251-2398  _minimize_scalar_bounded                  -> Powell::scalar_bounded
//     :2401-2573  Brent (get_bracket_info with brack=None)   -> Powell::scalar_brent
//     :2916-3072  bracket                                    -> Powell::bracket
//     :3079-3110  _recover_from_bracket_error                -> Powell::scalar_brent
//     :3113-3173  _line_for_search                           -> Powell::line_for_search
//     :3176-3230  _linesearch_powell                         -> Powell::linesearch
//     :3375-3614  _minimize_powell                           -> Powell::minimize
// Every sum, product and comparison is written in SciPy's order and form (a comparison with a
// NaN takes SciPy's branch), and the file must be compiled WITHOUT fused multiply-add
// (-ffp-contract=off): on the same objective values the search then evaluates the same points
// in the same order and returns the same bits (tests/test_host_powell.py, tests/test_gpu_powell.py).
//
// What Python does with an exception is done with `raised`: an evaluation requested when
// `fcalls >= maxfun` sets it, and every routine returns false at once; `minimize` then ends
// with x, fval and direc as they were before the interrupted line search would have assigned
// them (`except _MaxFuncCallError: break`).
//
// Bounds: none, or finite for every variable (`lower == upper` included).  With finite bounds
// `_line_for_search` yields an infinite limit only when a division overflows; SciPy would then
// go to its unbounded or its arctan line search, this file stays with `scalar_bounded`, whose
// own iteration cap ends it.  Every loop has SciPy's cap: `bracket` 1000 iterations, `Brent`
// and `_minimize_scalar_bounded` 500, and `minimize` its maxiter / maxfun, at least one of
// which is finite - every pass of its loop that does not end it evaluates the extrapolated
// point, so the evaluation budget alone bounds it too.
//
// KPDI_POWELL_COUNT (host tests only): every if / else arm and every loop exit of the routines
// above increments one entry of `kpdi_powell_count`.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KPDI_HD __host__ __device__
#else
#define KPDI_HD
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// clang-format off
#define KPDI_POWELL_BRANCHES(X)                                                                    \
  X(call_raise) X(call_ok)                                                                         \
  X(br_swap) X(br_noswap) X(br_exit_cond) X(br_small) X(br_large) X(br_cap)                        \
  X(br_between) X(br_between_lt_fc) X(br_between_gt_fb) X(br_between_neither)                      \
  X(br_limit) X(br_beyond) X(br_beyond_lt_fc) X(br_beyond_ge_fc) X(br_else)                        \
  X(br_invalid) X(br_valid)                                                                        \
  X(rec_nan) X(rec_argmin)                                                                         \
  X(bt_a_lt_c) X(bt_a_ge_c) X(bt_exit_cap) X(bt_exit_conv)                                         \
  X(bt_gold_hi) X(bt_gold_lo) X(bt_para) X(bt_para_neg) X(bt_para_pos)                             \
  X(bt_para_ok) X(bt_para_far) X(bt_para_edge) X(bt_para_edge_pos) X(bt_para_edge_neg)             \
  X(bt_para_bad_hi) X(bt_para_bad_lo)                                                              \
  X(bt_small) X(bt_small_pos) X(bt_small_neg) X(bt_step)                                           \
  X(bt_worse) X(bt_worse_left) X(bt_worse_right) X(bt_worse_second) X(bt_worse_third)              \
  X(bt_worse_none) X(bt_better) X(bt_better_right) X(bt_better_left)                               \
  X(bd_exit_cond) X(bd_exit_maxfun) X(bd_para) X(bd_nopara) X(bd_para_neg) X(bd_para_pos)          \
  X(bd_para_ok) X(bd_para_far) X(bd_para_edge) X(bd_para_bad)                                      \
  X(bd_golden) X(bd_nogolden) X(bd_gold_hi) X(bd_gold_lo)                                          \
  X(bd_better) X(bd_better_right) X(bd_better_left)                                                \
  X(bd_worse) X(bd_worse_left) X(bd_worse_right) X(bd_worse_second) X(bd_worse_third)              \
  X(bd_worse_none)                                                                                 \
  X(lfs_zero) X(lfs_nonzero) X(lfs_pos) X(lfs_neg) X(lfs_ok) X(lfs_empty)                          \
  X(ls_zero) X(ls_unbounded) X(ls_bounded)                                                         \
  X(pw_budget_default) X(pw_budget_maxfun) X(pw_budget_maxiter) X(pw_budget_both)                  \
  X(pw_bigger) X(pw_not_bigger) X(pw_exit_ftol) X(pw_exit_maxfun) X(pw_exit_maxiter)               \
  X(pw_exit_nan) X(pw_raise_in_set) X(pw_raise_new_direction) X(pw_lmax_one) X(pw_lmax_line)      \
  X(pw_extra_lower) X(pw_extra_not_lower) X(pw_t_neg) X(pw_t_nonneg)                               \
  X(pw_direc_replaced) X(pw_direc_kept)                                                            \
  X(pw_status_bounds) X(pw_status_maxfun) X(pw_status_maxiter) X(pw_status_nan) X(pw_status_ok)
// clang-format on

namespace kpdi {

enum PowellBranch {
#define KPDI_PW_ENUM(name) PWB_##name,
  KPDI_POWELL_BRANCHES(KPDI_PW_ENUM)
#undef KPDI_PW_ENUM
      PWB_COUNT
};

#ifdef KPDI_POWELL_COUNT
inline long long kpdi_powell_count[PWB_COUNT] = {};
inline const char *const kpdi_powell_branch_names[PWB_COUNT] = {
#define KPDI_PW_NAME(name) #name,
    KPDI_POWELL_BRANCHES(KPDI_PW_NAME)
#undef KPDI_PW_NAME
};
#define KPDI_PW_HIT(name) (++::kpdi::kpdi_powell_count[::kpdi::PWB_##name])
#else
#define KPDI_PW_HIT(name) ((void)0)
#endif

constexpr long long POWELL_UNLIMITED = 0x7fffffffffffffffLL;  // maxiter / maxfun = np.inf

// ---- NumPy's elementwise forms
KPDI_HD inline bool pw_isnan(double v) { return v != v; }
KPDI_HD inline bool pw_isfinite(double v) { return (v - v) == 0.0; }
KPDI_HD inline double pw_nan() { return __builtin_nan(""); }
// np.maximum / np.minimum and the np.max / np.min reductions: a NaN wins
KPDI_HD inline double pw_maximum(double a, double b) { return pw_isnan(a) ? a : (pw_isnan(b) ? b : (a > b ? a : b)); }
KPDI_HD inline double pw_minimum(double a, double b) { return pw_isnan(a) ? a : (pw_isnan(b) ? b : (a < b ? a : b)); }
// np.sign(v) + (v == 0)
KPDI_HD inline double pw_sign_or_one(double v) {
  const double sign = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : (v == 0.0 ? 0.0 : v));
  return sign + (v == 0.0 ? 1.0 : 0.0);
}

// E: `double eval(const double *x)`, the objective at n variables.
template <int NMAX, class E>
struct Powell {
  E &ev;
  int n;
  bool bounded, raised;
  double xtol, ftol;
  long long maxiter, maxfun, fcalls, iter;
  int status;
  double fval;
  double x[NMAX], lb[NMAX], ub[NMAX];
  double direc[NMAX][NMAX];

  KPDI_HD explicit Powell(E &e) : ev(e) {}

  // _wrap_scalar_function_maxfun_validation: false = _MaxFuncCallError was raised
  KPDI_HD bool call(const double *p, double *f) {
    if (fcalls >= maxfun) {
      KPDI_PW_HIT(call_raise);
      raised = true;
      return false;
    }
    KPDI_PW_HIT(call_ok);
    ++fcalls;
    *f = ev.eval(p);
    return true;
  }
  // myfunc of _linesearch_powell: func(p + alpha * xi)
  KPDI_HD bool along(const double *p, const double *xi, double alpha, double *f) {
    double t[NMAX];
    for (int i = 0; i < n; ++i) t[i] = p[i] + alpha * xi[i];
    return call(t, f);
  }

  // bracket(func, xa=0.0, xb=1.0, grow_limit=110.0, maxiter=1000); *valid = the three
  // conditions at its end hold and the iteration cap was not met
  KPDI_HD bool bracket(const double *p, const double *xi, double *pxa, double *pxb, double *pxc, double *pfa,
                       double *pfb, double *pfc, bool *valid) {
    const double gold = 1.618034, verysmall = 1e-21, grow_limit = 110.0;
    const int cap = 1000;
    double xa = 0.0, xb = 1.0, fa, fb;
    if (!along(p, xi, xa, &fa)) return false;
    if (!along(p, xi, xb, &fb)) return false;
    if (fa < fb) {
      KPDI_PW_HIT(br_swap);
      double t = xa; xa = xb; xb = t;
      t = fa; fa = fb; fb = t;
    } else {
      KPDI_PW_HIT(br_noswap);
    }
    double xc = xb + gold * (xb - xa), fc;
    if (!along(p, xi, xc, &fc)) return false;
    int it = 0;
    bool capped = false;
    for (;;) {
      if (!(fc < fb)) {
        KPDI_PW_HIT(br_exit_cond);
        break;
      }
      const double tmp1 = (xb - xa) * (fb - fc);
      const double tmp2 = (xb - xc) * (fb - fa);
      const double val = tmp2 - tmp1;
      double denom;
      if (std::fabs(val) < verysmall) {
        KPDI_PW_HIT(br_small);
        denom = 2.0 * verysmall;
      } else {
        KPDI_PW_HIT(br_large);
        denom = 2.0 * val;
      }
      double w = xb - ((xb - xc) * tmp2 - (xb - xa) * tmp1) / denom;
      const double wlim = xb + grow_limit * (xc - xb);
      if (it > cap) {
        KPDI_PW_HIT(br_cap);
        capped = true;
        break;
      }
      ++it;
      double fw;
      if ((w - xc) * (xb - w) > 0.0) {
        KPDI_PW_HIT(br_between);
        if (!along(p, xi, w, &fw)) return false;
        if (fw < fc) {
          KPDI_PW_HIT(br_between_lt_fc);
          xa = xb;
          xb = w;
          fa = fb;
          fb = fw;
          break;
        } else if (fw > fb) {
          KPDI_PW_HIT(br_between_gt_fb);
          xc = w;
          fc = fw;
          break;
        }
        KPDI_PW_HIT(br_between_neither);
        w = xc + gold * (xc - xb);
        if (!along(p, xi, w, &fw)) return false;
      } else if ((w - wlim) * (wlim - xc) >= 0.0) {
        KPDI_PW_HIT(br_limit);
        w = wlim;
        if (!along(p, xi, w, &fw)) return false;
      } else if ((w - wlim) * (xc - w) > 0.0) {
        KPDI_PW_HIT(br_beyond);
        if (!along(p, xi, w, &fw)) return false;
        if (fw < fc) {
          KPDI_PW_HIT(br_beyond_lt_fc);
          xb = xc;
          xc = w;
          w = xc + gold * (xc - xb);
          fb = fc;
          fc = fw;
          if (!along(p, xi, w, &fw)) return false;
        } else {
          KPDI_PW_HIT(br_beyond_ge_fc);
        }
      } else {
        KPDI_PW_HIT(br_else);
        w = xc + gold * (xc - xb);
        if (!along(p, xi, w, &fw)) return false;
      }
      xa = xb;
      xb = xc;
      xc = w;
      fa = fb;
      fb = fc;
      fc = fw;
    }
    const bool cond1 = (fb < fc && fb <= fa) || (fb < fa && fb <= fc);
    const bool cond2 = (xa < xb && xb < xc) || (xc < xb && xb < xa);
    const bool cond3 = pw_isfinite(xa) && pw_isfinite(xb) && pw_isfinite(xc);
    if (capped || !(cond1 && cond2 && cond3)) {
      KPDI_PW_HIT(br_invalid);
      *valid = false;
    } else {
      KPDI_PW_HIT(br_valid);
      *valid = true;
    }
    *pxa = xa; *pxb = xb; *pxc = xc;
    *pfa = fa; *pfb = fb; *pfc = fc;
    return true;
  }

  // _recover_from_bracket_error(_minimize_scalar_brent, myfunc, None, (), xtol=tol):
  // Brent(tol, maxiter=500).optimize() -> (xmin, fval)
  KPDI_HD bool scalar_brent(const double *p, const double *xi, double tol, double *xmin, double *fmin) {
    const double mintol = 1.0e-11, cg = 0.3819660;
    const int cap = 500;
    double xa, xb, xc, fa, fb, fc;
    bool valid;
    if (!bracket(p, xi, &xa, &xb, &xc, &fa, &fb, &fc, &valid)) return false;
    if (!valid) {
      if (pw_isnan(xa) || pw_isnan(xb) || pw_isnan(xc) || pw_isnan(fa) || pw_isnan(fb) || pw_isnan(fc)) {
        KPDI_PW_HIT(rec_nan);
        *xmin = pw_nan();
        *fmin = pw_nan();
      } else {
        KPDI_PW_HIT(rec_argmin);
        // np.argmin: the first of the smallest
        const bool b_first = fb < fa;
        const double x01 = b_first ? xb : xa, f01 = b_first ? fb : fa;
        const bool c_first = fc < f01;
        *xmin = c_first ? xc : x01;
        *fmin = c_first ? fc : f01;
      }
      return true;
    }
    double x = xb, w = xb, v = xb;
    double fw = fb, fv = fb, fx = fb;
    double a, b;
    if (xa < xc) {
      KPDI_PW_HIT(bt_a_lt_c);
      a = xa;
      b = xc;
    } else {
      KPDI_PW_HIT(bt_a_ge_c);
      a = xc;
      b = xa;
    }
    double deltax = 0.0, rat = 0.0;
    int it = 0;
    for (;;) {
      if (!(it < cap)) {
        KPDI_PW_HIT(bt_exit_cap);
        break;
      }
      const double tol1 = tol * std::fabs(x) + mintol;
      const double tol2 = 2.0 * tol1;
      const double xmid = 0.5 * (a + b);
      if (std::fabs(x - xmid) < (tol2 - 0.5 * (b - a))) {
        KPDI_PW_HIT(bt_exit_conv);
        break;
      }
      if (std::fabs(deltax) <= tol1) {
        if (x >= xmid) {
          KPDI_PW_HIT(bt_gold_hi);
          deltax = a - x;
        } else {
          KPDI_PW_HIT(bt_gold_lo);
          deltax = b - x;
        }
        rat = cg * deltax;
      } else {
        KPDI_PW_HIT(bt_para);
        const double tmp1 = (x - w) * (fx - fv);
        double tmp2 = (x - v) * (fx - fw);
        double pp = (x - v) * tmp2 - (x - w) * tmp1;
        tmp2 = 2.0 * (tmp2 - tmp1);
        if (tmp2 > 0.0) {
          KPDI_PW_HIT(bt_para_neg);
          pp = -pp;
        } else {
          KPDI_PW_HIT(bt_para_pos);
        }
        tmp2 = std::fabs(tmp2);
        const double dx_temp = deltax;
        deltax = rat;
        if ((pp > tmp2 * (a - x)) && (pp < tmp2 * (b - x)) && (std::fabs(pp) < std::fabs(0.5 * tmp2 * dx_temp))) {
          KPDI_PW_HIT(bt_para_ok);
          rat = pp * 1.0 / tmp2;
          const double u = x + rat;
          if ((u - a) < tol2 || (b - u) < tol2) {
            KPDI_PW_HIT(bt_para_edge);
            if (xmid - x >= 0.0) {
              KPDI_PW_HIT(bt_para_edge_pos);
              rat = tol1;
            } else {
              KPDI_PW_HIT(bt_para_edge_neg);
              rat = -tol1;
            }
          } else {
            KPDI_PW_HIT(bt_para_far);
          }
        } else {
          if (x >= xmid) {
            KPDI_PW_HIT(bt_para_bad_hi);
            deltax = a - x;
          } else {
            KPDI_PW_HIT(bt_para_bad_lo);
            deltax = b - x;
          }
          rat = cg * deltax;
        }
      }
      double u;
      if (std::fabs(rat) < tol1) {
        KPDI_PW_HIT(bt_small);
        if (rat >= 0.0) {
          KPDI_PW_HIT(bt_small_pos);
          u = x + tol1;
        } else {
          KPDI_PW_HIT(bt_small_neg);
          u = x - tol1;
        }
      } else {
        KPDI_PW_HIT(bt_step);
        u = x + rat;
      }
      double fu;
      if (!along(p, xi, u, &fu)) return false;
      if (fu > fx) {
        KPDI_PW_HIT(bt_worse);
        if (u < x) {
          KPDI_PW_HIT(bt_worse_left);
          a = u;
        } else {
          KPDI_PW_HIT(bt_worse_right);
          b = u;
        }
        if ((fu <= fw) || (w == x)) {
          KPDI_PW_HIT(bt_worse_second);
          v = w;
          w = u;
          fv = fw;
          fw = fu;
        } else if ((fu <= fv) || (v == x) || (v == w)) {
          KPDI_PW_HIT(bt_worse_third);
          v = u;
          fv = fu;
        } else {
          KPDI_PW_HIT(bt_worse_none);
        }
      } else {
        KPDI_PW_HIT(bt_better);
        if (u >= x) {
          KPDI_PW_HIT(bt_better_right);
          a = x;
        } else {
          KPDI_PW_HIT(bt_better_left);
          b = x;
        }
        v = w;
        w = x;
        x = u;
        fv = fw;
        fw = fx;
        fx = fu;
      }
      ++it;
    }
    *xmin = x;
    *fmin = fx;
    return true;
  }

  // _minimize_scalar_bounded(myfunc, (x1, x2), xatol, maxiter=500) -> (xf, fx)
  KPDI_HD bool scalar_bounded(const double *p, const double *xi, double x1, double x2, double xatol, double *xmin,
                              double *fmin) {
    const int maxfun_local = 500;
    const double sqrt_eps = std::sqrt(2.2e-16);
    const double golden_mean = 0.5 * (3.0 - std::sqrt(5.0));
    double a = x1, b = x2;
    double fulc = a + golden_mean * (b - a);
    double nfc = fulc, xf = fulc;
    double rat = 0.0, e = 0.0;
    double xx = xf, fx;
    if (!along(p, xi, xx, &fx)) return false;
    int num = 1;
    double ffulc = fx, fnfc = fx;
    double xm = 0.5 * (a + b);
    double tol1 = sqrt_eps * std::fabs(xf) + xatol / 3.0;
    double tol2 = 2.0 * tol1;
    for (;;) {
      if (!(std::fabs(xf - xm) > (tol2 - 0.5 * (b - a)))) {
        KPDI_PW_HIT(bd_exit_cond);
        break;
      }
      bool golden = true;
      if (std::fabs(e) > tol1) {
        KPDI_PW_HIT(bd_para);
        golden = false;
        double r = (xf - nfc) * (fx - ffulc);
        double q = (xf - fulc) * (fx - fnfc);
        double pp = (xf - fulc) * q - (xf - nfc) * r;
        q = 2.0 * (q - r);
        if (q > 0.0) {
          KPDI_PW_HIT(bd_para_neg);
          pp = -pp;
        } else {
          KPDI_PW_HIT(bd_para_pos);
        }
        q = std::fabs(q);
        r = e;
        e = rat;
        if ((std::fabs(pp) < std::fabs(0.5 * q * r)) && (pp > q * (a - xf)) && (pp < q * (b - xf))) {
          KPDI_PW_HIT(bd_para_ok);
          rat = (pp + 0.0) / q;
          xx = xf + rat;
          if (((xx - a) < tol2) || ((b - xx) < tol2)) {
            KPDI_PW_HIT(bd_para_edge);
            const double si = pw_sign_or_one(xm - xf);
            rat = tol1 * si;
          } else {
            KPDI_PW_HIT(bd_para_far);
          }
        } else {
          KPDI_PW_HIT(bd_para_bad);
          golden = true;
        }
      } else {
        KPDI_PW_HIT(bd_nopara);
      }
      if (golden) {
        KPDI_PW_HIT(bd_golden);
        if (xf >= xm) {
          KPDI_PW_HIT(bd_gold_hi);
          e = a - xf;
        } else {
          KPDI_PW_HIT(bd_gold_lo);
          e = b - xf;
        }
        rat = golden_mean * e;
      } else {
        KPDI_PW_HIT(bd_nogolden);
      }
      const double si = pw_sign_or_one(rat);
      xx = xf + si * pw_maximum(std::fabs(rat), tol1);
      double fu;
      if (!along(p, xi, xx, &fu)) return false;
      ++num;
      if (fu <= fx) {
        KPDI_PW_HIT(bd_better);
        if (xx >= xf) {
          KPDI_PW_HIT(bd_better_right);
          a = xf;
        } else {
          KPDI_PW_HIT(bd_better_left);
          b = xf;
        }
        fulc = nfc;
        ffulc = fnfc;
        nfc = xf;
        fnfc = fx;
        xf = xx;
        fx = fu;
      } else {
        KPDI_PW_HIT(bd_worse);
        if (xx < xf) {
          KPDI_PW_HIT(bd_worse_left);
          a = xx;
        } else {
          KPDI_PW_HIT(bd_worse_right);
          b = xx;
        }
        if ((fu <= fnfc) || (nfc == xf)) {
          KPDI_PW_HIT(bd_worse_second);
          fulc = nfc;
          ffulc = fnfc;
          nfc = xx;
          fnfc = fu;
        } else if ((fu <= ffulc) || (fulc == xf) || (fulc == nfc)) {
          KPDI_PW_HIT(bd_worse_third);
          fulc = xx;
          ffulc = fu;
        } else {
          KPDI_PW_HIT(bd_worse_none);
        }
      }
      xm = 0.5 * (a + b);
      tol1 = sqrt_eps * std::fabs(xf) + xatol / 3.0;
      tol2 = 2.0 * tol1;
      if (num >= maxfun_local) {
        KPDI_PW_HIT(bd_exit_maxfun);
        break;
      }
    }
    *xmin = xf;
    *fmin = fx;
    return true;
  }

  // _line_for_search(x0, alpha, lb, ub) -> (lmin, lmax).  np.max / np.min run over the entries
  // whose alpha is not zero; started from -inf / +inf they give the same values for any
  // non-empty set (an empty one makes SciPy raise ValueError; here it leaves the whole line).
  KPDI_HD void line_for_search(const double *x0, const double *alpha, double *plmin, double *plmax) {
    double lmin = -HUGE_VAL, lmax = HUGE_VAL;
    for (int i = 0; i < n; ++i) {
      if (alpha[i] == 0.0) {
        KPDI_PW_HIT(lfs_zero);
        continue;
      }
      KPDI_PW_HIT(lfs_nonzero);
      const double low = (lb[i] - x0[i]) / alpha[i];
      const double high = (ub[i] - x0[i]) / alpha[i];
      double vmin, vmax;
      if (alpha[i] > 0.0) {  // np.where(pos, low, 0) + np.where(pos, 0, high), ...
        KPDI_PW_HIT(lfs_pos);
        vmin = low + 0.0;
        vmax = high + 0.0;
      } else {
        KPDI_PW_HIT(lfs_neg);
        vmin = 0.0 + high;
        vmax = 0.0 + low;
      }
      lmin = pw_maximum(lmin, vmin);
      lmax = pw_minimum(lmax, vmax);
    }
    if (lmax >= lmin) {
      KPDI_PW_HIT(lfs_ok);
      *plmin = lmin;
      *plmax = lmax;
    } else {
      KPDI_PW_HIT(lfs_empty);
      *plmin = 0.0;
      *plmax = 0.0;
    }
  }

  // _linesearch_powell(func, p, xi, tol, lb, ub, fval) -> (fret, pnew, xinew); nothing is
  // written when an evaluation "raised"
  KPDI_HD bool linesearch(const double *p, const double *xi, double tol, double f_at_p, double *fret, double *pnew,
                          double *xinew) {
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || (xi[i] != 0.0);
    double alpha_min, f;
    if (!any) {
      KPDI_PW_HIT(ls_zero);
      *fret = f_at_p;
      for (int i = 0; i < n; ++i) {
        pnew[i] = p[i];
        xinew[i] = xi[i];
      }
      return true;
    } else if (!bounded) {
      KPDI_PW_HIT(ls_unbounded);
      if (!scalar_brent(p, xi, tol, &alpha_min, &f)) return false;
    } else {
      KPDI_PW_HIT(ls_bounded);
      double lmin, lmax;
      line_for_search(p, xi, &lmin, &lmax);
      if (!scalar_bounded(p, xi, lmin, lmax, tol / 100, &alpha_min, &f)) return false;
    }
    *fret = f;
    for (int i = 0; i < n; ++i) {
      const double s = alpha_min * xi[i];
      const double pi = p[i];
      xinew[i] = s;
      pnew[i] = pi + s;
    }
    return true;
  }

  // _minimize_powell(func, x0, bounds, xtol, ftol, maxiter, maxfev); max_iter / max_fev <= 0 =
  // None.  lower / upper: both null or both given.  Leaves x, fval, iter, fcalls, status.
  KPDI_HD void minimize(int nvar, const double *x0, const double *lower, const double *upper, double x_tol,
                        double f_tol, long long max_iter, long long max_fev) {
    n = nvar;
    xtol = x_tol;
    ftol = f_tol;
    bounded = lower != nullptr;
    raised = false;
    fcalls = 0;
    iter = 0;
    if (max_iter <= 0 && max_fev <= 0) {
      KPDI_PW_HIT(pw_budget_default);
      maxiter = (long long)n * 1000;
      maxfun = (long long)n * 1000;
    } else if (max_iter <= 0) {
      KPDI_PW_HIT(pw_budget_maxfun);
      maxiter = POWELL_UNLIMITED;
      maxfun = max_fev;
    } else if (max_fev <= 0) {
      KPDI_PW_HIT(pw_budget_maxiter);
      maxiter = max_iter;
      maxfun = POWELL_UNLIMITED;
    } else {
      KPDI_PW_HIT(pw_budget_both);
      maxiter = max_iter;
      maxfun = max_fev;
    }
    double x1[NMAX], d1[NMAX], xn[NMAX], dn[NMAX], x2[NMAX];
    for (int i = 0; i < n; ++i) {
      x[i] = x0[i];
      if (bounded) {
        lb[i] = lower[i];
        ub[i] = upper[i];
      }
      for (int j = 0; j < n; ++j) direc[i][j] = i == j ? 1.0 : 0.0;
    }
    call(x, &fval);  // maxfun >= 1: cannot raise
    for (int i = 0; i < n; ++i) x1[i] = x[i];
    const double tol = xtol * 100;
    for (;;) {
      const double fx = fval;
      int bigind = 0;
      double delta = 0.0;
      double fx2, fn;
      for (int i = 0; i < n && !raised; ++i) {
        for (int j = 0; j < n; ++j) d1[j] = direc[i][j];
        fx2 = fval;
        if (!linesearch(x, d1, tol, fval, &fn, xn, dn)) break;
        fval = fn;
        for (int j = 0; j < n; ++j) x[j] = xn[j];
        if ((fx2 - fval) > delta) {
          KPDI_PW_HIT(pw_bigger);
          delta = fx2 - fval;
          bigind = i;
        } else {
          KPDI_PW_HIT(pw_not_bigger);
        }
      }
      if (raised) {
        KPDI_PW_HIT(pw_raise_in_set);
        break;
      }
      ++iter;
      const double bnd = ftol * (std::fabs(fx) + std::fabs(fval)) + 1e-20;
      if (2.0 * (fx - fval) <= bnd) {
        KPDI_PW_HIT(pw_exit_ftol);
        break;
      }
      if (fcalls >= maxfun) {
        KPDI_PW_HIT(pw_exit_maxfun);
        break;
      }
      if (iter >= maxiter) {
        KPDI_PW_HIT(pw_exit_maxiter);
        break;
      }
      if (pw_isnan(fx) && pw_isnan(fval)) {
        KPDI_PW_HIT(pw_exit_nan);
        break;
      }
      // the extrapolated point
      for (int j = 0; j < n; ++j) {
        d1[j] = x[j] - x1[j];
        x1[j] = x[j];
      }
      double lmax;
      if (!bounded) {
        KPDI_PW_HIT(pw_lmax_one);
        lmax = 1.0;
      } else {
        KPDI_PW_HIT(pw_lmax_line);
        double lmin;
        line_for_search(x, d1, &lmin, &lmax);
      }
      const double step = 1.0 < lmax ? 1.0 : lmax;  // min(lmax, 1)
      for (int j = 0; j < n; ++j) x2[j] = x[j] + step * d1[j];
      call(x2, &fx2);  // cannot raise: fcalls < maxfun was tested above
      if (fx > fx2) {
        KPDI_PW_HIT(pw_extra_lower);
        double t = 2.0 * (fx + fx2 - 2.0 * fval);
        double temp = (fx - fval - delta);
        t *= temp * temp;
        temp = fx - fx2;
        t -= delta * temp * temp;
        if (t < 0.0) {
          KPDI_PW_HIT(pw_t_neg);
          if (!linesearch(x, d1, tol, fval, &fn, xn, dn)) {
            KPDI_PW_HIT(pw_raise_new_direction);
            break;
          }
          fval = fn;
          bool any = false;
          for (int j = 0; j < n; ++j) {
            x[j] = xn[j];
            any = any || (dn[j] != 0.0);
          }
          if (any) {
            KPDI_PW_HIT(pw_direc_replaced);
            for (int j = 0; j < n; ++j) direc[bigind][j] = direc[n - 1][j];
            for (int j = 0; j < n; ++j) direc[n - 1][j] = dn[j];
          } else {
            KPDI_PW_HIT(pw_direc_kept);
          }
        } else {
          KPDI_PW_HIT(pw_t_nonneg);
        }
      } else {
        KPDI_PW_HIT(pw_extra_not_lower);
      }
    }
    bool outside = false, xnan = false;
    for (int i = 0; i < n; ++i) {
      if (bounded) outside = outside || (lb[i] > x[i]) || (x[i] > ub[i]);
      xnan = xnan || pw_isnan(x[i]);
    }
    if (bounded && outside) {
      KPDI_PW_HIT(pw_status_bounds);
      status = 4;
    } else if (fcalls >= maxfun) {
      KPDI_PW_HIT(pw_status_maxfun);
      status = 1;
    } else if (iter >= maxiter) {
      KPDI_PW_HIT(pw_status_maxiter);
      status = 2;
    } else if (pw_isnan(fval) || xnan) {
      KPDI_PW_HIT(pw_status_nan);
      status = 3;
    } else {
      KPDI_PW_HIT(pw_status_ok);
      status = 0;
    }
  }
};

}  // namespace kpdi
