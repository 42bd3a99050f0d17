"""One table of LN_NELDERMEAD cases for the host test (csrc/nlopt_simplex.h compiled with the host compiler) and the
GPU test (`kpdi_nlopt_simplex_selftest`): every row runs through the header, the device kernel and the plain-Python
restatement of DESIGN.md section 21 (tests/_nlopt_simplex_restate.py), and all three must agree bit for bit.  NLopt
itself is not part of any of this (tools/compare_nlopt.py runs the table through it where it is installed).

The analytic objectives are those of tests/_powell_cases.py (kinds 0 to 4, in the operation order of
`AnalyticObjective`, csrc/analytic_objectives.h) and kind 5, `arms` (ANALYTIC_ARMS there): a sum of concave arms on
which contractions fail, so that the simplex shrinks."""

import collections
import math

import _nlopt_simplex_restate as restate
import _powell_cases as pc

INF = math.inf


def arms(x):
    acc = None
    for i in range(len(x)):
        d = abs(x[i] - 0.3 * float(i + 1))
        t = float(i + 1) * d / (1.0 + d)
        acc = t if acc is None else acc + t
    return float(acc)


OBJECTIVES = pc.OBJECTIVES + (arms,)

BOWL_BOX = ([0.5, 0.0, 0.0], [2.05, 1.5, 0.6])
BOX6 = ([0.0] * 6, [1, 1, 1.02, 1.2, 1.65, 2])
SMALLEST = 5e-324  # ftol_rel > 0 whose product with |fl| + |fh| < 0.5 is 0: only the `fl == fh` clause can hold

Case = collections.namedtuple("Case", "name kind x0 lower upper xstep ftol_rel maxeval expect")


def case(name, kind, x0, lower=None, upper=None, xstep=None, ftol_rel=1e-8, maxeval=0, **expect):
    """expect: status (name), phase (what the last evaluation was), nevals, hits (branches the row must reach)."""
    return Case(name, kind, x0, lower, upper, xstep, ftol_rel, maxeval, expect)


SHRINKING = dict(kind=5, x0=[2.0, -1.0, 0.5])  # evaluations: f sss r e r e r c r r c ... c sss (26-28) ...

CASES = [
    # sizes, unbounded and bounded
    # (a minimum of 0 never meets a RELATIVE tolerance: these end when the simplex has collapsed)
    case("bowl3", 1, [2.0, -1.0, 0.5], status="XTOL_REACHED", hits=["step_from_x", "contract_kept"]),
    case("rosen6", 0, [1.3, 0.7, 0.8, 1.9, 1.2, 0.5], xstep=[0.1] * 6, maxeval=300, hits=["step_given"]),
    case("bowl3_box", 1, [2.0, 1.0, 0.5], *BOWL_BOX, hits=["clamp_lower", "clamp_upper"]),
    case("bowl6_box", 1, [0.2, 0.5, 1.0, 1.1, 1.6, 1.7], *BOX6, maxeval=400),
    case("rosen2", 0, [-1.2, 1.0], ftol_rel=1e-6, status="XTOL_REACHED"),
    case("rosen1_of_2", 0, [-1.2, 1.0], [-2.0, 1.0], [2.0, 1.0], status="FTOL_REACHED", hits=["fe_held"]),
    # the start: a step that leaves the box
    case("above_far", 1, [1.0, 0.5], [0.0, 0.0], [1.2, 2.0], xstep=[0.5, 0.5], maxeval=3, hits=["st_above_far"]),
    case("above_near", 1, [1.19, 0.5], [0.0, 0.0], [1.2, 2.0], xstep=[0.5, 0.5], maxeval=3, hits=["st_above_near"]),
    case("below_far", 1, [1.0, 0.5], [0.8, 0.0], [3.0, 2.0], xstep=[-0.5, 0.5], maxeval=3, hits=["st_below_far"]),
    case("below_near", 1, [0.81, 0.5], [0.8, 0.0], [3.0, 2.0], xstep=[-0.5, 0.5], maxeval=3, hits=["st_below_near"]),
    case("reversed_outside_to_upper", 1, [0.81, 0.5], [0.8, 0.0], [1.0, 2.0], xstep=[-0.5, 0.5], maxeval=40,
         hits=["st_below_near", "st_reversed_outside"]),
    case("reversed_outside_to_lower", 1, [0.99, 0.5], [0.8, 0.0], [1.0, 2.0], xstep=[3.0, 0.5], maxeval=40,
         hits=["st_above_near", "st_below_near", "st_reversed_outside"]),
    case("above_then_below", 1, [1.19, 0.5], [1.0, 0.0], [1.2, 2.0], xstep=[0.5, 0.5], maxeval=40,
         hits=["st_above_near", "st_below_far"]),
    case("x0_on_lower", 1, [0.5, 0.0, 0.3], *BOWL_BOX, hits=["step_range"]),
    case("x0_on_upper", 1, [2.05, 1.5, 0.6], *BOWL_BOX, hits=["step_range"]),
    # one side only (the header takes a null array; the device entry is given infinities)
    case("upper_only", 1, [2.0, 1.0, 0.5], None, [2.05, 1.5, 0.6], maxeval=200, hits=["step_upper"]),
    case("lower_only", 1, [2.0, 1.0, 0.5], [1.9, 0.0, 0.45], None, maxeval=200, hits=["step_lower"]),
    # held variables
    case("one_held", 1, [2.0, 1.0, 0.5], [0.5, 1.0, 0.0], [2.05, 1.0, 0.6], hits=["fe_held", "fe_free"]),
    case("two_held", 0, [1.3, 0.7, 0.8], [1.3, -5.0, 0.8], [1.3, 5.0, 0.8], hits=["fe_held"]),
    case("all_held", 1, [2.0, 1.0, 0.5], [2.0, 1.0, 0.5], [2.0, 1.0, 0.5], status="SUCCESS", nevals=1, phase="held",
         hits=["fe_all_held"]),
    case("all_held_maxeval_1", 1, [2.0, 1.0, 0.5], [2.0, 1.0, 0.5], [2.0, 1.0, 0.5], maxeval=1, status="SUCCESS", nevals=1),
    # the default step, one rule per variable: range, upper, lower, x, 1, (range beaten by upper)
    case("default_steps", 1, [2.0, 1.0, 1.0, 1.5, 0.0, 3.9], [0.0, -INF, 0.5, -INF, -INF, 0.0],
         [4.0, 1.5, INF, INF, INF, 4.0], maxeval=200,
         hits=["step_range", "step_upper", "step_lower", "step_from_x", "step_one"]),
    case("default_step_infinite_arrays", 1, [2.0, 0.0], [-INF, -INF], [INF, INF], maxeval=60, hits=["step_from_x", "step_one"]),
    # refusals of the search itself
    case("zero_step", 1, [2.0, 1.0, 0.5], xstep=[0.1, 0.0, 0.1], status="FAILURE", nevals=2, hits=["st_no_move"]),
    case("outside_above", 1, [2.0, 1.0, 0.7], *BOWL_BOX, status="INVALID_ARGS", nevals=0, hits=["fe_invalid"]),
    case("outside_below", 1, [0.4, 1.0, 0.5], *BOWL_BOX, status="INVALID_ARGS", nevals=0),
    case("lower_above_upper", 1, [1.0, 1.0, 0.5], [0.5, 1.2, 0.0], [2.05, 0.8, 0.6], status="INVALID_ARGS", nevals=0),
    # maxeval on every CHECK position
    case("maxeval_first", maxeval=1, status="MAXEVAL_REACHED", nevals=1, phase="first", **SHRINKING),
    case("maxeval_start", maxeval=3, status="MAXEVAL_REACHED", nevals=3, phase="start", **SHRINKING),
    case("maxeval_reflection", maxeval=5, status="MAXEVAL_REACHED", nevals=5, phase="reflection", **SHRINKING),
    case("maxeval_expansion", maxeval=6, status="MAXEVAL_REACHED", nevals=6, phase="expansion", **SHRINKING),
    case("maxeval_contraction", maxeval=10, status="MAXEVAL_REACHED", nevals=10, phase="contraction", **SHRINKING),
    case("maxeval_shrink", maxeval=27, status="MAXEVAL_REACHED", nevals=27, phase="shrink", hits=["shrink"], **SHRINKING),
    case("shrink_and_on", maxeval=120, hits=["shrink", "expand_kept", "expand_rejected", "contract_inside",
                                               "contract_outside", "accept_reflection"], **SHRINKING),
    # the two clauses of the ftol test
    case("ftol_relative", 1, [2.0, 1.0, 0.5], *BOWL_BOX, ftol_rel=1e-3, status="FTOL_REACHED", hits=["ftol_relative"]),
    case("ftol_equal", 2, [0.5, 0.6, 0.9], xstep=[1e-9] * 3, ftol_rel=SMALLEST, status="FTOL_REACHED", nevals=4,
         hits=["ftol_equal", "tie_low", "tie_high"]),
    # collapse: the reflected point coincides with the centroid
    case("collapse", 1, [1.0, 1.0], xstep=[0.5, 0.5], ftol_rel=0.0, maxeval=2000, status="XTOL_REACHED",
         hits=["rf_coincides"]),
    case("collapse_1d", 1, [1.0], ftol_rel=0.0, maxeval=2000, status="XTOL_REACHED"),
    # ties: four equal values at the start (float32 plateau), then ties along the way
    case("ties_plateau", 2, [0.5, 0.6, 0.9], xstep=[1e-9] * 3, ftol_rel=0.0, maxeval=60, hits=["tie_low", "tie_high"]),
    case("ties_f32", 2, [2.0, -1.0, 0.5], ftol_rel=0.0, maxeval=250),
    # weights 1 and 4 of the bowl: steps 0.5 and 0.25 from their minima give the same float32 value at points 1 and 4
    case("ties_high", 2, [0.3, 1.0, 0.5, 1.2], xstep=[0.5, 0.1, 0.1, 0.25], ftol_rel=0.0, maxeval=30, hits=["tie_high"]),
    case("ties_symmetric", 1, [0.3, 0.6], xstep=[0.1, -0.1], lower=[0.2, 0.5], upper=[0.4, 0.7], ftol_rel=0.0, maxeval=50),
    # NaN objective values
    case("nan_region", 3, [1.0, 1.0, 0.5], xstep=[1.0, 0.5, 0.5], maxeval=150),
    case("nan_start", 3, [2.0, 1.0, 0.5], xstep=[-0.5, 0.5, 0.5], maxeval=150, hits=["ftol_not_finite"]),
    case("nan_region_box", 3, [1.0, 1.0, 0.5], *BOWL_BOX, maxeval=150),
    case("nan_everywhere", 4, [1.0, 1.0, 0.5], ftol_rel=1e-4, status="XTOL_REACHED", hits=["ftol_not_finite", "shrink"]),
    case("nan_everywhere_maxeval", 4, [1.0, 1.0, 0.5], *BOWL_BOX, maxeval=25, status="MAXEVAL_REACHED", nevals=25),
]

_WANT = {}


def want(i, variant=None):
    """The restatement's result of case i (computed once per variant)."""
    key = (i, variant)
    if key not in _WANT:
        c = CASES[i]
        _WANT[key] = restate.optimize(OBJECTIVES[c.kind], c.x0, c.lower, c.upper, c.xstep, c.ftol_rel, c.maxeval, variant)
    return _WANT[key]


same_bits = pc.same_bits
