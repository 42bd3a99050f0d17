"""One table of Powell cases for the host test (csrc/powell.h compiled with the host compiler) and the GPU test
(`kpdi_powell_selftest`), with the analytic objectives in the operation order of `AnalyticObjective`
(csrc/analytic_objectives.h), which both of them evaluate; this module is their independent statement: each row runs through `scipy.optimize.minimize(method="Powell")` and through the restatement, and the two must agree
bit for bit."""

import numpy as np
import scipy.optimize


def rosen(x):
    acc = None
    for i in range(len(x) - 1):
        d = x[i + 1] - x[i] * x[i]
        e = 1.0 - x[i]
        t = 100.0 * (d * d) + e * e
        acc = t if acc is None else acc + t
    return float(acc)


def bowl(x):
    acc = None
    for i in range(len(x)):
        d = x[i] - 0.3 * float(i + 1)
        t = float(i + 1) * (d * d)
        acc = t if acc is None else acc + t
    return float(acc)


def bowl_f32(x):
    """Plateaus and ties, like the float32 noise of the real objective."""
    return float(np.float32(bowl(x)))


def bowl_nan_region(x):
    return float("nan") if x[0] > 1.9 else bowl(x)


def all_nan(x):
    return float("nan")


OBJECTIVES = (rosen, bowl, bowl_f32, bowl_nan_region, all_nan)

BOX3 = ([0.5] * 3, [1.5] * 3)
BOWL_BOX = ([0.5, 0.0, 0.0], [2.05, 1.5, 0.6])
BOWL_FIXED = ([0.5, 1.0, 0.0], [2.05, 1.0, 0.6])
BOX6 = ([0.0] * 6, [1, 1, 1.02, 1.2, 1.65, 2])

# kind, x0, bounds (lower, upper) | None, options, what SciPy 1.15.3 returns: dict of nfev / nit / status where pinned
CASES = [
    (0, [-1.2, 1.0], None, {}, dict(nfev=607, nit=23)),
    (0, [1.3, 0.7, 0.8], None, {}, dict(nfev=478, nit=14)),                      # the direction set is replaced
    (0, [1.3, 0.7, 0.8, 1.9, 1.2, 0.5], None, {}, dict(nfev=1191, nit=18)),
    (0, [0.0, 0.0, 0.0], None, {}, dict(nfev=885)),
    (0, [1.3, 0.7, 0.8], BOX3, {}, dict(nfev=388)),
    (0, [3.0, 0.7, 0.8], BOX3, {}, dict(nfev=636)),                              # start outside the box
    (0, [1.3, 0.7, 0.8], None, dict(maxfev=37), dict(nfev=37, nit=1)),           # budget ends inside a line search
    (0, [1.3, 0.7, 0.8], None, dict(maxiter=2), dict(nfev=69, status=2)),
    (0, [1.3, 0.7, 0.8], BOX3, dict(maxfev=11), dict(nfev=11, nit=0)),
    (0, [1.3, 0.7, 0.8], None, dict(maxfev=1), dict(nfev=1)),
    (1, [2.0, -1.0, 0.5], None, dict(xtol=1e-8, ftol=1e-8), dict(nfev=48)),
    (1, [0.3, 0.6, 0.9], None, {}, dict(nfev=22)),                               # start at the minimum
    (1, [2.0, 1.0, 0.5], BOWL_BOX, {}, dict(nfev=139)),                          # minimum outside the box
    (1, [2.0, 1.0, 0.5], BOWL_FIXED, {}, dict(nfev=129)),                        # lower == upper for one variable
    (1, [2.0, 1.0, 0.5], BOWL_FIXED, dict(maxiter=1), dict(nfev=42)),
    (1, [0.2, 0.5, 1.0, 1.1, 1.6, 1.7], BOX6, {}, dict(nfev=104)),
    (2, [2.0, -1.0, 0.5], None, {}, dict(nfev=76)),
    (2, [2.0, 1.0, 0.5], BOWL_BOX, dict(xtol=1e-3, ftol=1e-3), dict(nfev=215)),
    (3, [1.0, 1.0, 0.5], None, {}, dict(nfev=20, status=3)),                     # x becomes NaN
    (3, [1.0, 1.0, 0.5], BOWL_BOX, {}, dict(nfev=94, status=0)),
    (4, [1.0, 1.0, 0.5], None, {}, dict(nfev=10)),
    (4, [1.0, 1.0, 0.5], BOWL_BOX, {}, dict(nfev=62)),
    # rows added for the branch test (tests/test_host_powell.py)
    (0, [1.3, 0.7, 0.8], None, dict(maxfev=69), dict(nfev=69, nit=2, status=1)),  # budget used up exactly at an iteration's end
    (0, [1.3, 0.7, 0.8], None, dict(maxfev=300, maxiter=3), dict(status=2)),      # both limits given
    (0, [3.0, 0.7, 0.8], BOX3, dict(maxfev=1), dict(nfev=1, status=4)),           # ends outside the box
    (1, [float("nan"), 1.0, 0.5], BOWL_BOX, {}, dict(status=3)),                  # NaN limits of the line: (0, 0)
    (0, [2.28, -1.35, 2.27], None, {}, {}),                                       # bracket: parabolic point neither better nor worse
    (0, [-1.82, 0.38, 0.07], None, {}, {}),                                       # bracket: parabolic point above f(xb)
    (1, [2.0, 1.0, 0.5], BOWL_BOX, dict(xtol=-1e-4, maxiter=1), dict(nfev=1501)),  # bounded search runs into its 500 evaluations
    (2, [1e9, 0.0, 0.0], None, {}, dict(nfev=10)),                               # float32 plateau: invalid bracket without a NaN
    (1, [0.5, 1.1, 0.6], BOWL_FIXED, {}, {}),                                     # new direction of length 0: direction set kept
    (0, [1.00000001, 0.99999999], None, dict(ftol=0.0, maxiter=4), {}),           # bracket on differences below 1e-21
]


def scipy_run(case):
    kind, x0, bounds, opt, _ = case
    kw = {}
    if bounds is not None:
        kw["bounds"] = list(zip(*bounds))
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "initial guess is not within the bounds", NaN results
        return scipy.optimize.minimize(OBJECTIVES[kind], np.array(x0, dtype=np.float64), method="Powell",
                                       options=dict(opt), **kw)


_WANT = {}


def want(i):
    """SciPy's result of case i, computed once."""
    if i not in _WANT:
        _WANT[i] = scipy_run(CASES[i])
    return _WANT[i]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """Bit for bit, any NaN equal to any NaN."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))
