// basinhopping.h - scipy.optimize.basinhopping of SciPy 1.15.3 around minimize(method="Nelder-Mead"), with the default
// step (RandomDisplacement under AdaptiveStepsize) and the default acceptance test (Metropolis), restated operation for
// operation in f64 for the host and the device (plain C++17, no HIP headers), over nelder_mead.h and the
// numpy.random.RandomState of differential_evolution.h.
//   scipy/optimize/_basinhopping.py
//     :18-38    Storage (the lowest result)                              -> BasinHopping::store
//     :64-97    BasinHoppingRunner.__init__ (the initial quench)         -> begin, quench_done (S_INITIAL)
//     :99-154   _monte_carlo_step                                        -> take_step, quench_done (S_HOP)
//     :156-182  one_cycle                                                -> quench_done (S_HOP)
//     :230-250  AdaptiveStepsize._adjust_step_size, take_step            -> take_step
//     :252-255  AdaptiveStepsize.report                                  -> quench_done (naccept)
//     :275-278  RandomDisplacement.__call__                              -> take_step
//     :313-336  Metropolis                                               -> begin (beta), metropolis
//     :693-734  basinhopping: niter_success, the loop, the result        -> begin, loop_tail, next_hop
//   scipy/optimize/_optimize.py:926-939  warnflag of _minimize_neldermead -> quench_success
// One RandomState(seed) serves the displacement and the acceptance test.  Per hop it is drawn from in this order:
// n times uniform(-stepsize, stepsize) in element order, then - after the quench - ONE uniform() for Metropolis, which
// is drawn even when w is 1.  Every sum, product and comparison is written in SciPy's order and form and the file must
// be compiled WITHOUT fused multiply-add: with the same seed and the same objective values the search then evaluates
// the same points in the same order and returns the same bits (tests/test_host_basinhopping.py,
// tests/test_gpu_basinhopping.py).  The one operation that need not round alike on the host and the device is the
// `exp` of Metropolis: its value w is only compared with the draw, and the tests choose inputs on which the two are
// never closer than 1e-12.
//
// Not restated: `take_step`, `accept_test`, `callback`, `disp`, a generator as `rng`, every local minimiser but
// Nelder-Mead and its `bounds` stay with SciPy on the host.  numpy raises OverflowError when a step size has grown
// until 2 * stepsize overflows; here the displacement becomes NaN.
//
// Like nelder_mead.h it is a state machine and not a loop: ONE thread owns it (and the stream) while the whole
// workgroup evaluates the objective.  After `begin` and after each `feed(f)` either `state == S_DONE` or `xeval()`
// holds the next point to evaluate.
//
// KPDI_BH_COUNT (host tests only): every if / else arm and every exit below increments one entry of `kpdi_bh_count`.
#pragma once

#include <cmath>
#include <cstdint>

#include "differential_evolution.h"
#include "nelder_mead.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// clang-format off
#define KPDI_BH_BRANCHES(X)                                                                                          \
  X(beta_inf) X(beta_finite) X(niter_success_default) X(niter_success_given)                                          \
  X(quench_maxfun) X(quench_maxiter) X(quench_ok) X(fun_nan) X(fun_number)                                            \
  X(init_failed) X(init_ok) X(hop_failed) X(hop_ok)                                                                   \
  X(adjust_not) X(adjust_up) X(adjust_down)                                                                           \
  X(metro_uphill) X(metro_not_uphill) X(accepted) X(rejected_draw) X(rejected_success)                                \
  X(store_new_failed) X(store_lower) X(store_best_failed) X(store_kept)                                               \
  X(count_reset) X(count_on)                                                                                          \
  X(exit_niter_success) X(exit_niter) X(exit_no_hop)
// clang-format on

namespace kpdi {

enum BhBranch {
#define KPDI_BH_ENUM(name) BHB_##name,
  KPDI_BH_BRANCHES(KPDI_BH_ENUM)
#undef KPDI_BH_ENUM
      BHB_COUNT
};

#ifdef KPDI_BH_COUNT
inline long long kpdi_bh_count[BHB_COUNT] = {};
inline const char *const kpdi_bh_branch_names[BHB_COUNT] = {
#define KPDI_BH_NAME(name) #name,
    KPDI_BH_BRANCHES(KPDI_BH_NAME)
#undef KPDI_BH_NAME
};
#define KPDI_BH_HIT(name) (++::kpdi::kpdi_bh_count[::kpdi::BHB_##name])
#else
#define KPDI_BH_HIT(name) ((void)0)
#endif

template <int NV>
struct BasinHopping {
  enum { S_INITIAL, S_HOP, S_DONE };
  NelderMead<NV> nm;  // the quench that runs
  int n, state;
  // the options
  int niter, interval, maxiter, maxfun;
  long long niter_success;
  double beta, stepsize, target_accept_rate, factor, xatol, fatol;
  // BasinHoppingRunner: x, incumbent_minres (its fun and success)
  double x[NV], incumbent_fun;
  bool incumbent_success;
  // AdaptiveStepsize
  long long nstep, naccept;
  // the loop of `basinhopping`
  long long count;
  int i;
  // the result: Storage.minres (fun, x, success) and the counters of BasinHoppingRunner.res
  double fun, xbest[NV];
  bool success;
  long long nfev;
  int nit, minimization_failures;

  KPDI_HD const double *xeval() const { return nm.xeval; }

  // warnflag == 0 of _minimize_neldermead: fcalls >= maxfun is looked at first, then iterations >= maxiter
  KPDI_HD bool quench_success() const {
    if (nm.fcalls >= nm.maxfun) {
      KPDI_BH_HIT(quench_maxfun);
      return false;
    }
    if (nm.iterations >= nm.maxiter) {
      KPDI_BH_HIT(quench_maxiter);
      return false;
    }
    KPDI_BH_HIT(quench_ok);
    return true;
  }

  // fval = np.min(fsim): a NaN among the values is the minimum (the values are sorted, NaN last)
  KPDI_HD double quench_fun() const {
    if (nm.fsim[n] != nm.fsim[n]) {
      KPDI_BH_HIT(fun_nan);
      return nm.fsim[n];
    }
    KPDI_BH_HIT(fun_number);
    return nm.fun();
  }

  // Storage.update: true = a new global minimum
  KPDI_HD bool store(const double *xq, double fq, bool ok) {
    if (!ok) {
      KPDI_BH_HIT(store_new_failed);
      return false;
    }
    if (fq < fun) {
      KPDI_BH_HIT(store_lower);
    } else if (!success) {
      KPDI_BH_HIT(store_best_failed);
    } else {
      KPDI_BH_HIT(store_kept);
      return false;
    }
    fun = fq;
    success = ok;
    for (int k = 0; k < n; ++k) xbest[k] = xq[k];
    return true;
  }

  // Metropolis.accept_reject: w = exp(min(0, prod)), where Python's min(0, prod) is prod only if prod < 0 - a NaN
  // (a NaN energy; 0 * inf at T = 0 on equal energies) gives w = 1.  The draw is made whatever w is.
  KPDI_HD bool metropolis(Mt19937 &mt, double f_new, bool ok_new) {
    const double prod = -(f_new - incumbent_fun) * beta;
    double w;
    if (prod < 0.0) {
      KPDI_BH_HIT(metro_uphill);
      w = std::exp(prod);
    } else {
      KPDI_BH_HIT(metro_not_uphill);
      w = 1.0;
    }
    const double rand = mt_uniform(mt, 0.0, 1.0);
    if (!(w >= rand)) {
      KPDI_BH_HIT(rejected_draw);
      return false;
    }
    if (!(ok_new || !incumbent_success)) {
      KPDI_BH_HIT(rejected_success);
      return false;
    }
    KPDI_BH_HIT(accepted);
    return true;
  }

  // AdaptiveStepsize.take_step around RandomDisplacement, then the quench from the displaced point
  KPDI_HD void take_step(Mt19937 &mt) {
    ++nstep;
    if (nstep % (long long)interval == 0) {
      const double accept_rate = (double)naccept / (double)nstep;
      if (accept_rate > target_accept_rate) {
        KPDI_BH_HIT(adjust_up);
        stepsize /= factor;
      } else {
        KPDI_BH_HIT(adjust_down);
        stepsize *= factor;
      }
    } else {
      KPDI_BH_HIT(adjust_not);
    }
    double x_after_step[NV];
    for (int k = 0; k < n; ++k) x_after_step[k] = x[k] + mt_uniform(mt, -stepsize, stepsize);
    state = S_HOP;
    nm.begin(n, x_after_step, nullptr, nullptr, xatol, fatol, maxiter, maxfun);
  }

  // `for i in range(niter)`: the next cycle, or the result
  KPDI_HD void next_hop(Mt19937 &mt) {
    if (i < niter) return take_step(mt);
    if (niter > 0) {
      KPDI_BH_HIT(exit_niter);
      nit = niter;  // i + 1 with the last i of the loop
    } else {
      KPDI_BH_HIT(exit_no_hop);
      nit = 1;  // i = 0 from before the loop
    }
    state = S_DONE;
  }

  // a quench has ended: nm holds its result
  KPDI_HD void quench_done(Mt19937 &mt) {
    const bool ok = quench_success();
    const double fq = quench_fun();
    const double *xq = nm.sim[0];
    if (state == S_INITIAL) {
      if (!ok) {
        KPDI_BH_HIT(init_failed);
        ++minimization_failures;
      } else {
        KPDI_BH_HIT(init_ok);
      }
      for (int k = 0; k < n; ++k) x[k] = xbest[k] = xq[k];
      incumbent_fun = fun = fq;
      incumbent_success = success = ok;
      nfev = nm.fcalls;
      count = 0;
      i = 0;
      return next_hop(mt);
    }
    if (!ok) {
      KPDI_BH_HIT(hop_failed);
      ++minimization_failures;
    } else {
      KPDI_BH_HIT(hop_ok);
    }
    nfev += nm.fcalls;
    const bool accept = metropolis(mt, fq, ok);
    bool new_global_min = false;
    if (accept) {
      ++naccept;  // AdaptiveStepsize.report
      for (int k = 0; k < n; ++k) x[k] = xq[k];
      incumbent_fun = fq;
      incumbent_success = ok;
      new_global_min = store(xq, fq, ok);
    }
    ++count;
    if (new_global_min) {
      KPDI_BH_HIT(count_reset);
      count = 0;
    } else if (count > niter_success) {
      KPDI_BH_HIT(exit_niter_success);
      nit = i + 1;
      state = S_DONE;
      return;
    } else {
      KPDI_BH_HIT(count_on);
    }
    ++i;
    next_hop(mt);
  }

  KPDI_HD void advance(Mt19937 &mt) {
    while (state != S_DONE && nm.state == NelderMead<NV>::S_DONE) quench_done(mt);
  }

  // basinhopping(func, x0, niter, T, stepsize, minimizer_kwargs = Nelder-Mead with (xatol, fatol, max_iter, max_fun:
  // the resolved budget, both >= 1), interval >= 1, niter_success (< 0: None), target_accept_rate, stepwise_factor) on
  // the stream `mt`, which the caller has seeded
  KPDI_HD void begin(Mt19937 &mt, int nvar, const double *x0, int niter_, double T, double stepsize_, int interval_,
                     long long niter_success_, double target_accept_rate_, double stepwise_factor, double xa, double fa,
                     int max_iter, int max_fun) {
    n = nvar;
    niter = niter_;
    interval = interval_;
    stepsize = stepsize_;
    target_accept_rate = target_accept_rate_;
    factor = stepwise_factor;
    xatol = xa;
    fatol = fa;
    maxiter = max_iter;
    maxfun = max_fun;
    if (T != 0.0) {
      KPDI_BH_HIT(beta_finite);
      beta = 1.0 / T;
    } else {
      KPDI_BH_HIT(beta_inf);
      beta = HUGE_VAL;
    }
    if (niter_success_ < 0) {
      KPDI_BH_HIT(niter_success_default);
      niter_success = (long long)niter + 2;
    } else {
      KPDI_BH_HIT(niter_success_given);
      niter_success = niter_success_;
    }
    nstep = naccept = 0;
    minimization_failures = 0;
    nfev = 0;
    nit = 0;
    state = S_INITIAL;
    nm.begin(n, x0, nullptr, nullptr, xatol, fatol, maxiter, maxfun);
    advance(mt);
  }

  KPDI_HD void feed(Mt19937 &mt, double f) {
    nm.feed(f);
    advance(mt);
  }
};

}  // namespace kpdi
