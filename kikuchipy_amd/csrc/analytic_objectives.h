// analytic_objectives.h - the analytic f64 objectives on which the optimiser headers (nelder_mead.h, powell.h,
// nlopt_simplex.h, differential_evolution.h) are pinned, for the host and the device (plain C++17, no HIP headers): the
// self-test kernels of refine.hip and the drivers of the host tests evaluate THIS text.  The independent statement of the
// same functions is the Python of tests/_powell_cases.py, tests/_nlopt_simplex_cases.py and tests/_de_cases.py, which
// SciPy runs; the two must agree bit for bit, so every sum and product here keeps the order written there and the file
// must be compiled without fused multiply-add.
//
// Kinds 0..4 mean the same to every self-test.  Kind 5 does not: kpdi_nlopt_simplex_selftest's 5 is `arms`,
// kpdi_de_selftest's 5 is `hug` (its 6 and 7 are ANALYTIC_INF and ANALYTIC_CONSTANT).  Here each function has one
// number; `analytic_kind_de` maps the differential-evolution numbering onto it.
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

namespace kpdi {

enum AnalyticKind {
  ANALYTIC_ROSENBROCK = 0,  // sum(100 (x[i+1] - x[i]^2)^2 + (1 - x[i])^2)
  ANALYTIC_BOWL = 1,        // sum((i + 1) (x[i] - 0.3 (i + 1))^2)
  ANALYTIC_BOWL_F32 = 2,    // the bowl rounded to float32 and back: plateaus and ties, like the real objective's noise
  ANALYTIC_BOWL_NAN = 3,    // the bowl, NaN where x[0] > 1.9
  ANALYTIC_NAN = 4,         // NaN everywhere
  ANALYTIC_ARMS = 5,        // sum((i + 1) |d| / (1 + |d|)), d = x[i] - 0.3 (i + 1): concave arms, contractions fail
  ANALYTIC_INF = 6,         // +inf everywhere
  ANALYTIC_CONSTANT = 7,    // 0.1 everywhere
  ANALYTIC_HUG = 8,         // sum((i + 1) (d d + 0.1 d)), d = |x[i]|: the minimum sits on the lower bound of a box from 0
};

// kpdi_de_selftest and tests/_de_cases.py: 0..4 as everywhere, 5 = hug, 6 = +inf, 7 = 0.1
KPDI_HD inline int analytic_kind_de(int kind) { return kind == 5 ? ANALYTIC_HUG : kind; }

// The `E` of the optimiser headers: `eval(x)` at n variables.
struct AnalyticObjective {
  int kind, n;
  KPDI_HD double eval(const double *x) const {
    if (kind == ANALYTIC_NAN || (kind == ANALYTIC_BOWL_NAN && x[0] > 1.9)) return __builtin_nan("");
    if (kind == ANALYTIC_INF) return HUGE_VAL;
    if (kind == ANALYTIC_CONSTANT) return 0.1;
    double acc = 0.0;
    if (kind == ANALYTIC_ROSENBROCK) {
      for (int i = 0; i + 1 < n; ++i) {
        const double d = x[i + 1] - x[i] * x[i], e = 1.0 - x[i];
        const double t = 100.0 * (d * d) + e * e;
        acc = i == 0 ? t : acc + t;
      }
    } else if (kind == ANALYTIC_ARMS) {
      for (int i = 0; i < n; ++i) {
        const double d = std::fabs(x[i] - 0.3 * (double)(i + 1));
        const double t = (double)(i + 1) * d / (1.0 + d);
        acc = i == 0 ? t : acc + t;
      }
    } else if (kind == ANALYTIC_HUG) {
      for (int i = 0; i < n; ++i) {
        const double d = std::fabs(x[i]);
        const double t = (double)(i + 1) * (d * d + 0.1 * d);
        acc = i == 0 ? t : acc + t;
      }
    } else {  // the bowl and its variants
      for (int i = 0; i < n; ++i) {
        const double d = x[i] - 0.3 * (double)(i + 1);
        const double t = (double)(i + 1) * (d * d);
        acc = i == 0 ? t : acc + t;
      }
    }
    return kind == ANALYTIC_BOWL_F32 ? (double)(float)acc : acc;
  }
};

}  // namespace kpdi
