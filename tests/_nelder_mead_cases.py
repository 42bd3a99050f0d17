"""One table of Nelder-Mead cases for the host test (csrc/nelder_mead.h compiled with the host compiler) and the GPU test
(`kpdi_nelder_mead_selftest`), on the analytic objectives of tests/_powell_cases.py (kinds 0 to 4; their C++ statement
is csrc/analytic_objectives.h): each row runs through `scipy.optimize.minimize(method="Nelder-Mead")` and through the
restatement, and the two must agree bit for bit."""

import warnings

import numpy as np
import scipy.optimize

import _powell_cases as pc

OBJECTIVES = pc.OBJECTIVES

same_bits = pc.same_bits

BOWL_BOX = ([0.5, 0.0, 0.0], [2.05, 1.5, 0.6])
BOWL_FIXED = ([0.5, 1.0, 0.0], [2.05, 1.0, 0.6])
BOX6 = ([0, 0, 0, 0, 0, 0], [1, 1, 1.02, 1.2, 1.65, 2])
ROSEN3 = [1.3, 0.7, 0.8]
SHRINKS = [-2.12, 0.25, 0.33]

# kind, x0, bounds (lower, upper) | None, options
CASES = [
    (0, [-1.2, 1.0], None, {}),
    (0, [1.3, 0.7, 0.8], None, {}),
    (0, [1.3, 0.7, 0.8, 1.9, 1.2, 0.5], None, {}),
    (0, [0.0, 0.0, 0.0], None, {}),                                   # zero entries: the 0.00025 step
    (1, [2.0, -1.0, 0.5], None, dict(xatol=1e-8, fatol=1e-8)),
    (1, [2.0, 1.0, 0.5], ([0.5, 0.0, 0.0], [2.05, 1.5, 0.6]), {}),      # minimum outside the box; reflection at ub
    (1, [0.2, 0.5, 1.0, 1.1, 1.6, 1.7], ([0, 0, 0, 0, 0, 0], [1, 1, 1.02, 1.2, 1.65, 2]), {}),
    (0, [1.3, 0.7, 0.8], None, dict(maxfev=37)),                       # evaluation budget hit mid-iteration
    (0, [1.3, 0.7, 0.8], None, dict(maxiter=25)),
    (0, [1.3, 0.7, 0.8, 1.9, 1.2, 0.5], None, dict(maxfev=11, maxiter=500)),
    (0, [1.3, 0.7, 0.8], None, dict(maxfev=3)),                        # budget smaller than the initial simplex
    # float32 plateaus and ties
    (2, [2.0, -1.0, 0.5], None, {}),
    (2, [1e9, 0.0, 0.0], None, {}),                                    # plateau: the spread of the values is 0 at once
    (2, [0.3, 0.6, 0.9], None, dict(xatol=1e-12, fatol=1e-12)),        # started at the minimum, tolerances below float32
    # NaN in a region: started inside the finite region, next to the NaN region, inside it
    (3, [1.0, 1.0, 0.5], None, {}),
    (3, [1.85, 1.0, 0.5], None, {}),                                   # the first vertex of the simplex is NaN
    (3, [2.5, 1.0, 1.0], None, {}),                                    # every value NaN: runs to its budget
    (3, [2.5, 1.0, 1.0], BOWL_BOX, {}),
    (4, [1.0, 2.0], None, {}),                                         # NaN everywhere: runs to its budget
    (4, [1.0, 2.0], None, dict(maxiter=30)),
    # one variable
    (1, [2.0], None, {}),
    (2, [-3.0], ([-4.0], [0.1]), {}),
    # lower == upper for one variable; a start on a bound; a start outside the box
    (1, [2.0, 1.0, 0.5], BOWL_FIXED, {}),
    (1, [2.05, 0.0, 0.3], BOWL_BOX, {}),
    (0, [3.0, 0.7, 0.8], ([0.5] * 3, [1.5] * 3), {}),
    # rows added for the branch test (tests/test_host_nelder_mead.py)
    (0, SHRINKS, None, {}),                                            # an outside contraction fails: shrink
    (0, ROSEN3, None, dict(xatol=10.0, fatol=1e-12)),                  # the simplex is small enough, its values are not
    # ... the budget ends before the expansion, the outside and the inside contraction, and inside a shrink
    (0, ROSEN3, None, dict(maxfev=5)),
    (0, ROSEN3, None, dict(maxfev=13)),
    (0, ROSEN3, None, dict(maxfev=15)),
    (0, SHRINKS, None, dict(maxfev=21)),
    (0, SHRINKS, None, dict(maxfev=22)),
]


def scipy_run(case):
    kind, x0, bounds, opt = case
    kw = {}
    if bounds is not None:
        kw["bounds"] = list(zip(*bounds))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "initial guess is not within the bounds", NaN results
        return scipy.optimize.minimize(OBJECTIVES[kind], np.array(x0, dtype=np.float64), method="Nelder-Mead",
                                       options=dict(opt), **kw)


_WANT = {}


def want(i):
    """SciPy's result of case i, computed once."""
    if i not in _WANT:
        _WANT[i] = scipy_run(CASES[i])
    return _WANT[i]
