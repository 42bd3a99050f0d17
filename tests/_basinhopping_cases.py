"""One table of basinhopping cases for the host test (csrc/basinhopping.h compiled with the host compiler) and the GPU
test (`kpdi_basinhopping_selftest`), on the analytic objectives of tests/_powell_cases.py (kinds 0..4, in the operation
order of `AnalyticObjective` in csrc/analytic_objectives.h): each row runs through
`scipy.optimize.basinhopping(fun, x0, seed=..., minimizer_kwargs=dict(method="Nelder-Mead", ...), **kw)` and through
the restatement, and the two must agree bit for bit.

The one operation of the search that need not round alike everywhere is the `exp` of the Metropolis test, whose value
w is only compared with a uniform draw.  `replay` records (w, draw) of every hop of a SciPy run, and `margin_ok`
asserts |w - draw| > 1e-12 wherever 0 < w < 1: a condition on the inputs chosen here, not a tolerance of a comparison.

Also the small inputs of the real objective (the shapes of tests/test_gpu_de.py) for the public calls."""

import math
import warnings
from unittest import mock

import numpy as np
import scipy.optimize
from scipy.optimize import _basinhopping as _bh

import _powell_cases as pc

OBJECTIVES = pc.OBJECTIVES   # 0 rosen, 1 bowl, 2 bowl_f32, 3 bowl, NaN where x[0] > 1.9, 4 NaN everywhere
same_bits = pc.same_bits
INT_MAX = 2**31 - 1
MARGIN = 1e-12


def nm(**options):
    """minimizer_kwargs of a Nelder-Mead quench with these options."""
    return dict(method="Nelder-Mead", options=options) if options else dict(method="Nelder-Mead")


# kind, x0, keyword arguments of basinhopping (seed and minimizer_kwargs among them), what SciPy 1.15.3 returns where
# pinned (the premises are asserted in tests/test_host_basinhopping.py)
CASES = [
    # the defaults around a default quench, three and six variables
    (1, [1.0, 1.0, 1.0], dict(seed=0, niter=8, minimizer_kwargs=nm()), dict(nit=8, success=True, failures=0)),
    (0, [1.3, 0.7, 0.8, 1.9, 1.2, 0.5], dict(seed=1, niter=3, minimizer_kwargs=nm()), dict(nit=3)),
    # one variable, the largest seed, the step size adjusted every second hop
    (1, [2.0], dict(seed=2**32 - 1, niter=12, interval=2, minimizer_kwargs=nm()), dict(nit=12, both_ways=True)),
    # T = 0: uphill is never taken (w = 0), a tie (0 * inf) always; bowl_f32 ties
    (2, [0.5, 0.5, 0.5], dict(seed=2, niter=10, T=0, interval=2, minimizer_kwargs=nm(xatol=1e-2, fatol=1e-2)),
     dict(nit=10)),
    (1, [0.2, 0.9], dict(seed=3, niter=6, T=0, minimizer_kwargs=nm()), dict(nit=6)),
    # niter_success stops the loop early
    (1, [1.0, 1.0, 1.0], dict(seed=4, niter=30, niter_success=2, minimizer_kwargs=nm()), dict(early=True)),
    (1, [0.4], dict(seed=5, niter=9, niter_success=0, minimizer_kwargs=nm()), dict(early=True)),
    # quench budgets so small that no quench succeeds: by evaluations, by iterations, both given
    (0, [-1.2, 1.0, 0.5], dict(seed=6, niter=5, minimizer_kwargs=nm(maxfev=30)), dict(nit=5, success=False, failures=6)),
    (0, [-1.2, 1.0, 0.5], dict(seed=7, niter=5, stepsize=0.2, minimizer_kwargs=nm(maxiter=12)),
     dict(nit=5, success=False, failures=6)),
    (0, [-1.2, 1.0], dict(seed=8, niter=4, T=0.05, minimizer_kwargs=nm(maxiter=40, maxfev=45)), dict(nit=4, success=False)),
    # a budget on the edge: some quenches succeed and some fail (both clauses of the acceptance and of the storage)
    (1, [0.5, 0.5, 0.5], dict(seed=9, niter=20, interval=3, stepsize=1.0, minimizer_kwargs=nm(maxfev=118)),
     dict(nit=20, mixed=True)),
    (1, [3.0, -2.0, 4.0], dict(seed=10, niter=12, T=5.0, stepsize=0.1, minimizer_kwargs=nm(maxfev=150)),
     dict(nit=12, mixed=True)),
    # no hop at all
    (1, [1.0, 1.0, 1.0], dict(seed=11, niter=0, minimizer_kwargs=nm()), dict(nit=1, success=True, failures=0)),
    (4, [1.0, 1.0], dict(seed=12, niter=0, minimizer_kwargs=nm(maxfev=9)), dict(nit=1, success=False, failures=1, nfev=9)),
    # NaN everywhere: never a success, every quench ends by its budget, every hop is accepted (w = 1, nothing succeeded)
    (4, [0.3, 0.6, 0.9], dict(seed=13, niter=3, minimizer_kwargs=nm(maxfev=20)),
     dict(nit=3, success=False, failures=4, nfev=80)),
    (4, [0.3, 0.6, 0.9, 1.2, 1.5, 1.8], dict(seed=14, niter=2, interval=1, minimizer_kwargs=nm(maxiter=5)),
     dict(nit=2, success=False, failures=3)),
    # NaN in a region: the initial quench fails inside it (NaN energy), a later one succeeds outside
    (3, [2.2, 0.5, 0.5], dict(seed=15, niter=8, stepsize=0.6, minimizer_kwargs=nm(maxfev=200)), dict(nit=8, success=True)),
    # tol sets xatol and fatol; other rates and factors
    (1, [0.0, 0.0], dict(seed=16, niter=9, interval=2, target_accept_rate=0.9, stepwise_factor=0.5,
                         minimizer_kwargs=dict(method="Nelder-Mead", tol=1e-7)), dict(nit=9)),
    (0, [0.8, 0.9, 1.1], dict(seed=17, niter=7, interval=2, T=1e-4, target_accept_rate=0.1, stepwise_factor=0.7,
                              minimizer_kwargs=nm(xatol=1e-3, fatol=1e-3, maxfev=120)), dict(nit=7)),
]

# the cases the GPU self-test runs: one and six variables, T = 0, the adjusted step, the early stop, failing quenches,
# no hop, NaN
GPU_CASES = [0, 1, 2, 3, 5, 7, 10, 12, 14, 15, 16]


def quench_options(case):
    """(xatol, fatol, maxiter, maxfev) of the case's quench as `scipy.optimize.minimize` resolves `tol` and `options`."""
    mk = case[2]["minimizer_kwargs"]
    options, tol = dict(mk.get("options") or {}), mk.get("tol")
    default = 1e-4 if tol is None else tol
    return (options.get("xatol", default), options.get("fatol", default), options.get("maxiter"), options.get("maxfev"))


def budget(n, maxiter, maxfev):
    """The budget of _minimize_neldermead (scipy/optimize/_optimize.py:798-812); unlimited = INT_MAX."""
    if maxiter is None and maxfev is None:
        return 200 * n, 200 * n
    if maxiter is None:
        return INT_MAX, maxfev
    if maxfev is None:
        return maxiter, INT_MAX
    return maxiter, maxfev


def replay(fun, x0, **kw):
    """`scipy.optimize.basinhopping(fun, x0, **kw)` and (w, draw) of every hop: Metropolis is wrapped, it computes and
    draws exactly as it does unwrapped."""
    hops = []
    original = _bh.Metropolis.accept_reject

    def recorded(self, res_new, res_old):
        state = self.rng.get_state()
        out = original(self, res_new, res_old)
        prod = -(float(res_new.fun) - float(res_old.fun)) * self.beta
        w = math.exp(prod) if prod < 0 else 1.0
        rs = np.random.RandomState()
        rs.set_state(state)
        draw = rs.uniform()
        assert bool(out) == (w >= draw and bool(res_new.success or not res_old.success))
        hops.append((w, draw))
        return out

    with warnings.catch_warnings(), mock.patch.object(_bh.Metropolis, "accept_reject", recorded):
        warnings.simplefilter("ignore")  # NaN energies
        res = scipy.optimize.basinhopping(fun, np.array(x0, dtype=np.float64), **kw)
    return res, hops


def margin_ok(hops):
    """The condition on the inputs: where 0 < w < 1, w and the draw are further apart than any rounding of exp."""
    return all(abs(w - draw) > MARGIN for w, draw in hops if 0 < w < 1)


_WANT = {}


def want(i):
    """SciPy's result of case i and its hops, computed once."""
    if i not in _WANT:
        kind, x0, kw, _ = CASES[i]
        _WANT[i] = replay(OBJECTIVES[kind], x0, **kw)
    return _WANT[i]


def step_sizes(case):
    """The step size before every hop of the case, from the acceptances of its SciPy run (a check of the table only:
    does the step size move both ways?)."""
    kw = case[2]
    out, nstep, naccept, size = [], 0, 0, kw.get("stepsize", 0.5)
    accepts = []
    original = _bh.AdaptiveStepsize.report

    def report(self, accept, **kwargs):
        accepts.append(bool(accept))
        return original(self, accept, **kwargs)

    with warnings.catch_warnings(), mock.patch.object(_bh.AdaptiveStepsize, "report", report):
        warnings.simplefilter("ignore")
        scipy.optimize.basinhopping(OBJECTIVES[case[0]], np.array(case[1], dtype=np.float64), **kw)
    for accept in accepts:
        nstep += 1
        if nstep % kw.get("interval", 50) == 0:
            if naccept / nstep > kw.get("target_accept_rate", 0.5):
                size /= kw.get("stepwise_factor", 0.9)
            else:
                size *= kw.get("stepwise_factor", 0.9)
        out.append(size)
        naccept += accept
    return out


# ---- the real objective: the shapes of tests/test_gpu_de.py
BH = dict(seed=7, niter=5, stepsize=0.02, T=0.01, interval=2,
          minimizer_kwargs=dict(method="Nelder-Mead", options=dict(maxfev=50)))


def real_inputs():
    """A 41 x 41 two-hemisphere Lambert master pattern, a 6 x 8 detector with a signal mask (41 kept pixels: no multiple
    of anything), three patterns - the last one constant, whose centred pattern is zero and whose objective is NaN at
    every point (never a success, every quench ends by its budget) - starts a degree off and one pseudo-symmetry
    operator (two starts per pattern)."""
    import kikuchipy_amd as ka
    from kikuchipy_amd.indexing._refinement import rotation_from_euler

    y, x = np.mgrid[-1:1:41j, -1:1:41j]
    upper = np.cos(3 * x + 0.5) * np.sin(2 * y - 0.3) + 0.3 * np.cos(5 * x * y) + 0.2 * x
    lower = np.sin(2 * x - 0.2) * np.cos(3 * y + 0.1) + 0.3 * np.sin(4 * x * y) - 0.2 * y
    mp = ka.EBSDMasterPattern(np.stack([upper, lower]).astype(np.float32), phase_name="ni")
    det = ka.EBSDDetector(shape=(6, 8), pc=(0.42, 0.55, 0.5), sample_tilt=70)
    euler = np.array([[0.9, 0.7, 0.4], [2.1, 1.1, 1.3], [4.0, 0.5, 2.2]])
    sim = np.asarray(mp.get_patterns(rotation_from_euler(euler), det).data.compute(), dtype=np.float64).reshape(3, 6, 8)
    sim = (sim - sim.min()) / (sim.max() - sim.min())
    pats = np.clip(np.round(sim * 255), 0, 255).astype(np.uint8)
    pats[2] = 100
    rot0 = rotation_from_euler(euler + np.deg2rad([[1.0, -0.8, 0.6], [-0.7, 0.9, 1.0], [0.5, 0.5, -0.5]]))
    mask = np.zeros((6, 8), dtype=bool)
    mask[0, :3] = mask[5, 6:] = mask[2, 4] = mask[3, 1] = True
    op = np.array([[np.cos(np.deg2rad(5)), 0, 0, np.sin(np.deg2rad(5))]])
    return ka.EBSD(pats), det, mp, rot0, mask, op
