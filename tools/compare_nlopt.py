"""Run the case table of tests/_nlopt_simplex_cases.py through an installed NLopt (`nlopt.opt(nlopt.LN_NELDERMEAD, n)`)
and through the restatement the device solver is pinned to (tests/_nlopt_simplex_restate.py), and print where the two
part ways: per case the status, the number of evaluations, the lowest value and the point, and the index of the first
evaluation at which the two asked for different points.

This is the one comparison the test suite cannot make: NLopt is not a dependency and is absent where the suite runs.
The tool installs nothing and fetches nothing; without the `nlopt` module it says so and exits.

    python tools/compare_nlopt.py"""

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def nlopt_run(nlopt, case, objective):
    """(status, nevals, minf, x, evaluated points) of the case in NLopt; an exception becomes its result code."""
    import numpy as np

    n = len(case.x0)
    opt = nlopt.opt(nlopt.LN_NELDERMEAD, n)
    points = []

    def f(x, grad):
        points.append([float(v) for v in x])
        return objective(points[-1])

    opt.set_min_objective(f)
    opt.set_ftol_rel(case.ftol_rel)
    if case.lower is not None:
        opt.set_lower_bounds(case.lower)
    if case.upper is not None:
        opt.set_upper_bounds(case.upper)
    if case.xstep is not None:
        opt.set_initial_step(case.xstep)
    if case.maxeval > 0:
        opt.set_maxeval(case.maxeval)
    try:
        x = opt.optimize(np.array(case.x0, dtype=np.float64))
        return opt.last_optimize_result(), opt.get_numevals(), opt.last_optimum_value(), [float(v) for v in x], points
    except ValueError:   # nlopt invalid argument
        return -2, len(points), float("inf"), list(case.x0), points
    except RuntimeError:  # nlopt failure
        return -1, len(points), float("nan"), list(case.x0), points


def main():
    try:
        import nlopt
    except ImportError:
        print("the nlopt module is not installed: nothing was compared")
        return 0
    import _nlopt_simplex_cases as nc
    import _nlopt_simplex_restate as restate

    apart = 0
    for i, case in enumerate(nc.CASES):
        objective = nc.OBJECTIVES[case.kind]
        asked = []

        def traced(x, objective=objective, asked=asked):
            asked.append(list(x))
            return objective(x)

        want = restate.optimize(traced, case.x0, case.lower, case.upper, case.xstep, case.ftol_rel, case.maxeval)
        status, nevals, minf, x, points = nlopt_run(nlopt, case, objective)
        first = next((k for k, (a, b) in enumerate(zip(asked, points)) if not nc.same_bits(a, b)), None)
        if first is None and len(asked) != len(points):
            first = min(len(asked), len(points))
        same = (first is None and (status, nevals) == (want.status, want.nevals) and nc.same_bits(x, want.x)
                and nc.same_bits(minf, want.minf))
        apart += not same
        print(f"{case.name}: {'same' if same else 'APART'}")
        if not same:
            print(f"  restatement: status {want.status} nevals {want.nevals} minf {want.minf!r} x {want.x}")
            print(f"  nlopt {nlopt.__version__}: status {status} nevals {nevals} minf {minf!r} x {x}")
            if first is not None:
                a = asked[first] if first < len(asked) else None
                b = points[first] if first < len(points) else None
                print(f"  first different evaluation: {first}: restatement {a}, nlopt {b}")
    print(f"{len(nc.CASES) - apart} of {len(nc.CASES)} cases the same, {apart} apart")
    return 1 if apart else 0


if __name__ == "__main__":
    sys.exit(main())
