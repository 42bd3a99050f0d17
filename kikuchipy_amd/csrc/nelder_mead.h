// nelder_mead.h - scipy.optimize.minimize(method="Nelder-Mead") of SciPy 1.15.3 (not adaptive, no initial_simplex, no
// callback), restated operation for operation in f64 for the host and the device (plain C++17, no HIP headers).
//   scipy/optimize/_optimize.py
//     :530-554  _wrap_scalar_function_maxfun_validation      -> NelderMead::request
//     :682-949  _minimize_neldermead
//       :769-783  x0 clipped, the initial simplex              -> NelderMead::begin
//       :814-824  vertices above the upper bound reflected     -> NelderMead::begin
//       :831-844  the first N + 1 values, argsort              -> NelderMead::feed (S_INIT), NelderMead::sort
//       :848-852  the loop's condition and termination test    -> NelderMead::loop_top
//       :854-858  centroid and reflected point                 -> NelderMead::loop_top
//       :861-901  expansion, the two contractions              -> NelderMead::feed
//       :903-909  shrink                                       -> NelderMead::shrink_step, NelderMead::feed (S_SHRINK)
//       :910-916  iterations += 1, `finally:` argsort          -> NelderMead::end_iteration, NelderMead::raised
//       :923-924  x = sim[0], fval = np.min(fsim)              -> NelderMead::sim[0], NelderMead::fun
// The budget of :798-812 (both unset: 200 N each; one unset: that one unlimited) is resolved by the caller
// (`resolve_budget` in extras.hip); `begin` takes the two numbers.
// Every sum, product and comparison is written in SciPy's order and form, and the file must be compiled WITHOUT fused
// multiply-add (-ffp-contract=off): on the same objective values the search then evaluates the same points in the same
// order and returns the same bits (tests/test_host_nelder_mead.py, tests/test_gpu_refinement.py).
//
// The search is a state machine and not a loop, because on the device ONE thread owns it while the whole workgroup
// evaluates the objective: `begin` and `feed(f)` are called by that one thread, and after each call either
// `state == S_DONE` or `xeval` holds the next point to evaluate.  What Python does with `_MaxFuncCallError` is done by
// `request` returning false: the caller of `request` goes to `raised`, the `finally:` sort and the loop's condition,
// which then ends the search (fcalls >= maxfun).
//
// The termination test, `np.max(|sim[1:] - sim[0]|) <= xatol and np.max(|fsim[0] - fsim[1:]|) <= fatol`, keeps a NaN
// as np.max does: a NaN among the differences makes it false, and the search runs on to its budget as SciPy's does.
// It is written as "every difference <= the tolerance", which is the same predicate for finite values and for NaN (a
// comparison with a NaN is false, as is the comparison of a NaN maximum) and costs the one thread that runs it a
// compare per element, where a NaN-keeping maximum costs two compares and a select.  (With fmax, which drops a NaN, a
// simplex whose values are all NaN had a spread of 0 and ended as soon as it was small.)
//
// KPDI_NELDER_MEAD_COUNT (host tests only): every if / else arm of `begin`, `request`, `loop_top`, `feed` and
// `shrink_step`, and every exit, increments one entry of `kpdi_nelder_mead_count`.
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
#define KPDI_NELDER_MEAD_BRANCHES(X)                                                               \
  X(rq_raise) X(rq_ok)                                                                             \
  X(bg_bounded) X(bg_unbounded) X(bg_zero_entry) X(bg_nonzero_entry)                               \
  X(bg_above_upper) X(bg_not_above_upper) X(bg_first_raise) X(bg_first_ok)                         \
  X(lt_spread_x) X(lt_spread_f) X(lt_reflect_ok) X(lt_reflect_raise)                               \
  X(fd_init_next) X(fd_init_full) X(fd_init_raise)                                                 \
  X(fd_expand) X(fd_expand_raise) X(fd_reflect_kept)                                               \
  X(fd_contract_out) X(fd_contract_out_raise) X(fd_contract_in) X(fd_contract_in_raise)            \
  X(fd_expanded) X(fd_expand_failed)                                                               \
  X(fd_contracted_out) X(fd_contract_out_failed) X(fd_contracted_in) X(fd_contract_in_failed)      \
  X(fd_shrink_next) X(fd_shrink_full)                                                              \
  X(sh_ok) X(sh_raise)                                                                             \
  X(exit_maxfun) X(exit_maxiter) X(exit_converged)
// clang-format on

namespace kpdi {

enum NelderMeadBranch {
#define KPDI_NM_ENUM(name) NMB_##name,
  KPDI_NELDER_MEAD_BRANCHES(KPDI_NM_ENUM)
#undef KPDI_NM_ENUM
      NMB_COUNT
};

#ifdef KPDI_NELDER_MEAD_COUNT
inline long long kpdi_nelder_mead_count[NMB_COUNT] = {};
inline const char *const kpdi_nelder_mead_branch_names[NMB_COUNT] = {
#define KPDI_NM_NAME(name) #name,
    KPDI_NELDER_MEAD_BRANCHES(KPDI_NM_NAME)
#undef KPDI_NM_NAME
};
#define KPDI_NM_HIT(name) (++::kpdi::kpdi_nelder_mead_count[::kpdi::NMB_##name])
#else
#define KPDI_NM_HIT(name) ((void)0)
#endif

template <int NV>
struct NelderMead {
  enum { S_INIT, S_REFLECT, S_EXPAND, S_CONTRACT_OUT, S_CONTRACT_IN, S_SHRINK, S_DONE };
  int n, state, j, fcalls, iterations, maxiter, maxfun, bounded;
  double xatol, fatol;
  double sim[NV + 1][NV], fsim[NV + 1];
  double lb[NV], ub[NV];
  double xbar[NV], xr[NV], xt[NV], fxr;
  double xeval[NV];

  KPDI_HD void clip(double *x) const {
    if (!bounded) return;
    for (int i = 0; i < n; ++i) x[i] = std::fmin(std::fmax(x[i], lb[i]), ub[i]);  // np.clip
  }
  // the evaluation-count guard of _wrap_scalar_function_maxfun_validation: false = "raised"
  KPDI_HD bool request(const double *x) {
    if (fcalls >= maxfun) {
      KPDI_NM_HIT(rq_raise);
      return false;
    }
    KPDI_NM_HIT(rq_ok);
    ++fcalls;
    for (int i = 0; i < n; ++i) xeval[i] = x[i];
    return true;
  }
  // np.argsort on <= 7 values = insertion sort: stable, NaN last
  KPDI_HD void sort() {
    for (int a = 1; a <= n; ++a) {
      const double f = fsim[a];
      double x[NV];
      for (int i = 0; i < n; ++i) x[i] = sim[a][i];
      int b = a - 1;
      while (b >= 0 && (f < fsim[b] || (fsim[b] != fsim[b] && f == f))) {
        fsim[b + 1] = fsim[b];
        for (int i = 0; i < n; ++i) sim[b + 1][i] = sim[b][i];
        --b;
      }
      fsim[b + 1] = f;
      for (int i = 0; i < n; ++i) sim[b + 1][i] = x[i];
    }
  }
  KPDI_HD void finish() { state = S_DONE; }
  KPDI_HD void raised() {  // `except _MaxFuncCallError: pass` + `finally:` sort
    sort();
    loop_top();
  }
  KPDI_HD void end_iteration() {
    ++iterations;
    sort();
    loop_top();
  }
  KPDI_HD void accept(const double *x, double f) {
    for (int i = 0; i < n; ++i) sim[n][i] = x[i];
    fsim[n] = f;
  }
  KPDI_HD void loop_top() {
    if (!(fcalls < maxfun && iterations < maxiter)) {
      if (fcalls >= maxfun)
        KPDI_NM_HIT(exit_maxfun);
      else
        KPDI_NM_HIT(exit_maxiter);
      return finish();
    }
    bool x_small = true, f_small = true;  // np.max(...) <= tol: every element is, and none is NaN
    for (int a = 1; a <= n; ++a) {
      for (int i = 0; i < n; ++i) x_small &= std::fabs(sim[a][i] - sim[0][i]) <= xatol;
      f_small &= std::fabs(fsim[0] - fsim[a]) <= fatol;
    }
    if (x_small && f_small) {
      KPDI_NM_HIT(exit_converged);
      return finish();
    }
    if (!x_small)
      KPDI_NM_HIT(lt_spread_x);
    else
      KPDI_NM_HIT(lt_spread_f);
    for (int i = 0; i < n; ++i) {
      double s = sim[0][i];
      for (int a = 1; a < n; ++a) s += sim[a][i];  // np.add.reduce(sim[:-1], 0)
      xbar[i] = s / (double)n;
      xr[i] = 2.0 * xbar[i] - 1.0 * sim[n][i];  // (1 + rho) * xbar - rho * sim[-1]
    }
    clip(xr);
    state = S_REFLECT;
    if (!request(xr)) {
      KPDI_NM_HIT(lt_reflect_raise);
      raised();
    } else {
      KPDI_NM_HIT(lt_reflect_ok);
    }
  }
  KPDI_HD void shrink_step() {
    for (int i = 0; i < n; ++i) sim[j][i] = sim[0][i] + 0.5 * (sim[j][i] - sim[0][i]);
    clip(sim[j]);
    state = S_SHRINK;
    if (!request(sim[j])) {
      KPDI_NM_HIT(sh_raise);
      raised();
    } else {
      KPDI_NM_HIT(sh_ok);
    }
  }
  // lower / upper: both null or both given.  max_iter, max_fun: the resolved budget, both >= 1
  KPDI_HD void begin(int nvar, const double *x0, const double *lower, const double *upper, double xa, double fa,
                     int max_iter, int max_fun) {
    n = nvar;
    xatol = xa;
    fatol = fa;
    maxiter = max_iter;
    maxfun = max_fun;
    bounded = lower != nullptr;
    double x[NV];
    for (int i = 0; i < n; ++i) {
      x[i] = x0[i];
      if (bounded) {
        lb[i] = lower[i];
        ub[i] = upper[i];
      }
    }
    clip(x);
    for (int i = 0; i < n; ++i) sim[0][i] = x[i];
    for (int k = 0; k < n; ++k) {
      for (int i = 0; i < n; ++i) sim[k + 1][i] = x[i];
      if (x[k] != 0.0)
        KPDI_NM_HIT(bg_nonzero_entry);
      else
        KPDI_NM_HIT(bg_zero_entry);
      sim[k + 1][k] = x[k] != 0.0 ? (1.0 + 0.05) * x[k] : 0.00025;
    }
    if (bounded) {  // reflect vertices above the upper bound into the interior, then clip
      KPDI_NM_HIT(bg_bounded);
      for (int a = 0; a <= n; ++a) {
        for (int i = 0; i < n; ++i)
          if (sim[a][i] > ub[i]) {
            KPDI_NM_HIT(bg_above_upper);
            sim[a][i] = 2.0 * ub[i] - sim[a][i];
          } else {
            KPDI_NM_HIT(bg_not_above_upper);
          }
        clip(sim[a]);
      }
    } else {
      KPDI_NM_HIT(bg_unbounded);
    }
    for (int a = 0; a <= n; ++a) fsim[a] = HUGE_VAL;
    fcalls = 0;
    iterations = 1;
    state = S_INIT;
    j = 0;
    if (!request(sim[0])) {
      KPDI_NM_HIT(bg_first_raise);
      sort();
      loop_top();
    } else {
      KPDI_NM_HIT(bg_first_ok);
    }
  }
  KPDI_HD void feed(double f) {
    switch (state) {
      case S_INIT:
        fsim[j] = f;
        ++j;
        if (j <= n) {
          if (request(sim[j])) {
            KPDI_NM_HIT(fd_init_next);
            return;
          }
          KPDI_NM_HIT(fd_init_raise);  // the budget is smaller than the initial simplex
        } else {
          KPDI_NM_HIT(fd_init_full);
        }
        sort();
        loop_top();
        return;
      case S_REFLECT:
        fxr = f;
        if (fxr < fsim[0]) {
          KPDI_NM_HIT(fd_expand);
          for (int i = 0; i < n; ++i) xt[i] = 3.0 * xbar[i] - 2.0 * sim[n][i];  // (1 + rho chi) xbar - rho chi sim[-1]
          clip(xt);
          state = S_EXPAND;
          if (!request(xt)) {
            KPDI_NM_HIT(fd_expand_raise);
            raised();
          }
        } else if (fxr < fsim[n - 1]) {
          KPDI_NM_HIT(fd_reflect_kept);
          accept(xr, fxr);
          end_iteration();
        } else if (fxr < fsim[n]) {
          KPDI_NM_HIT(fd_contract_out);
          for (int i = 0; i < n; ++i) xt[i] = 1.5 * xbar[i] - 0.5 * sim[n][i];  // (1 + psi rho) xbar - psi rho sim[-1]
          clip(xt);
          state = S_CONTRACT_OUT;
          if (!request(xt)) {
            KPDI_NM_HIT(fd_contract_out_raise);
            raised();
          }
        } else {
          KPDI_NM_HIT(fd_contract_in);
          for (int i = 0; i < n; ++i) xt[i] = 0.5 * xbar[i] + 0.5 * sim[n][i];  // (1 - psi) xbar + psi sim[-1]
          clip(xt);
          state = S_CONTRACT_IN;
          if (!request(xt)) {
            KPDI_NM_HIT(fd_contract_in_raise);
            raised();
          }
        }
        return;
      case S_EXPAND:
        if (f < fxr) {
          KPDI_NM_HIT(fd_expanded);
          accept(xt, f);
        } else {
          KPDI_NM_HIT(fd_expand_failed);
          accept(xr, fxr);
        }
        end_iteration();
        return;
      case S_CONTRACT_OUT:
        if (f <= fxr) {
          KPDI_NM_HIT(fd_contracted_out);
          accept(xt, f);
          end_iteration();
        } else {
          KPDI_NM_HIT(fd_contract_out_failed);
          j = 1;
          shrink_step();
        }
        return;
      case S_CONTRACT_IN:
        if (f < fsim[n]) {
          KPDI_NM_HIT(fd_contracted_in);
          accept(xt, f);
          end_iteration();
        } else {
          KPDI_NM_HIT(fd_contract_in_failed);
          j = 1;
          shrink_step();
        }
        return;
      case S_SHRINK:
        fsim[j] = f;
        ++j;
        if (j <= n) {
          KPDI_NM_HIT(fd_shrink_next);
          shrink_step();
        } else {
          KPDI_NM_HIT(fd_shrink_full);
          end_iteration();
        }
        return;
      default:
        return;
    }
  }
  // OptimizeResult: fun = np.min(fsim), x = sim[0]
  KPDI_HD double fun() const {
    double m = fsim[0];
    for (int a = 1; a <= n; ++a) m = fsim[a] < m ? fsim[a] : m;
    return m;
  }
};

}  // namespace kpdi
