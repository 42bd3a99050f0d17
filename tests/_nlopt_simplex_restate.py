"""The LN_NELDERMEAD search of DESIGN.md section 21 in plain Python float64, written from that text (not from
csrc/nlopt_simplex.h): the front end, CHECK, the start and the loop, with the same named branches counted.

`optimize(f, x0, lower, upper, xstep, ftol_rel, maxeval, variant=None)` returns a `Result`.  `variant` selects one of
three deliberately WRONG readings of the text, which tests/test_host_nlopt_simplex.py shows the case table to catch:
  "tie_rule"     the low point is the HIGHER storage index among equals, the high point the LOWER
  "clamp_order"  the upper clamp before the lower one, in `reflect` (where it cannot matter while lower <= upper, and the
                 front end lets nothing else through) and in the start, where a reversed step is then never brought
                 back into the box
  "check_order"  CHECK compares nevals with maxeval before it increments nevals
Python floats are IEEE doubles and `a + b * c` is never fused, so the arithmetic is that of the header built with
-ffp-contract=off.
"""

import collections
import math

FAILURE, INVALID_ARGS, SUCCESS, FTOL_REACHED, XTOL_REACHED, MAXEVAL_REACHED = -1, -2, 1, 3, 4, 5
STATUS_NAMES = {FAILURE: "FAILURE", INVALID_ARGS: "INVALID_ARGS", SUCCESS: "SUCCESS", FTOL_REACHED: "FTOL_REACHED",
                XTOL_REACHED: "XTOL_REACHED", MAXEVAL_REACHED: "MAXEVAL_REACHED"}
INF = math.inf

BRANCHES = """fe_invalid fe_held fe_free fe_all_held
step_given step_range step_upper step_lower step_from_x step_one
chk_better chk_not_better chk_maxeval
st_plain st_above_far st_above_near st_below_far st_below_near st_reversed_outside st_no_move
tie_low tie_high
ftol_relative ftol_equal ftol_not_finite ftol_go_on
clamp_lower clamp_upper rf_coincides rf_ok
expand expand_kept expand_rejected accept_reflection
contract_inside contract_outside contract_kept shrink""".split()

# phase: what the LAST evaluation was - first | start | reflection | expansion | contraction | shrink | held (None: none)
Result = collections.namedtuple("Result", "status nevals minf x counts phase")


class _Stop(Exception):
    pass


def close(a, b):
    return abs(a - b) <= 1e-13 * (abs(a) + abs(b))


def tiny(v):
    return v == 0 or abs(v) < 2.2250738585072014e-308


def optimize(f, x0, lower=None, upper=None, xstep=None, ftol_rel=0.0, maxeval=0, variant=None):
    counts = collections.Counter()
    nvar = len(x0)
    x0 = [float(v) for v in x0]
    lower = [-INF] * nvar if lower is None else [float(v) for v in lower]
    upper = [INF] * nvar if upper is None else [float(v) for v in upper]
    state = dict(status=SUCCESS, nevals=0, minf=INF, x=list(x0), phase=None)

    def done():
        return Result(state["status"], state["nevals"], state["minf"], state["x"], counts, state["phase"])

    # ------------------------------------------------------------ front end
    if any(x0[i] < lower[i] or x0[i] > upper[i] for i in range(nvar)):
        counts["fe_invalid"] += 1
        state["status"] = INVALID_ARGS
        return done()
    held = [lower[i] == upper[i] for i in range(nvar)]
    free = [i for i in range(nvar) if not held[i]]
    counts["fe_held"] += nvar - len(free)
    counts["fe_free"] += len(free)
    base = [lower[i] if held[i] else x0[i] for i in range(nvar)]
    state["x"] = list(base)
    n = len(free)

    def full(p):
        out = list(base)
        for k, i in enumerate(free):
            out[i] = p[k]
        return out

    if n == 0:
        counts["fe_all_held"] += 1
        state["phase"] = "held"
        state["minf"] = f(base)
        state["nevals"] = 1
        return done()

    lb = [lower[i] for i in free]
    ub = [upper[i] for i in free]
    start = [x0[i] for i in free]
    if xstep is not None:
        counts["step_given"] += n
        step = [float(xstep[i]) for i in free]
    else:
        step = []
        for k in range(n):
            s = INF
            if not math.isinf(ub[k]) and not math.isinf(lb[k]) and ub[k] > lb[k] and (ub[k] - lb[k]) * 0.25 < s:
                counts["step_range"] += 1
                s = (ub[k] - lb[k]) * 0.25
            if not math.isinf(ub[k]) and ub[k] > start[k] and ub[k] - start[k] < s:
                counts["step_upper"] += 1
                s = (ub[k] - start[k]) * 0.75
            if not math.isinf(lb[k]) and start[k] > lb[k] and start[k] - lb[k] < s:
                counts["step_lower"] += 1
                s = (start[k] - lb[k]) * 0.75
            if math.isinf(s) or tiny(s):
                counts["step_from_x"] += 1
                s = start[k]
            if math.isinf(s) or tiny(s):
                counts["step_one"] += 1
                s = 1.0
            step.append(s)

    # ------------------------------------------------------------ CHECK
    def check(value, point):
        if variant == "check_order":
            hit = maxeval > 0 and state["nevals"] >= maxeval
            state["nevals"] += 1
        else:
            state["nevals"] += 1
            hit = maxeval > 0 and state["nevals"] >= maxeval
        if value < state["minf"]:
            counts["chk_better"] += 1
            state["minf"] = value
            state["x"] = full(point)
        else:
            counts["chk_not_better"] += 1
        if hit:
            counts["chk_maxeval"] += 1
            state["status"] = MAXEVAL_REACHED
            raise _Stop

    def evaluate(point, phase):
        state["phase"] = phase
        value = f(full(point))
        check(value, point)
        return value

    def reflect(centre, scale, xold):
        """The reflected point; XTOL_REACHED when it coincides with the centre or with xold."""
        out = []
        for i in range(n):
            v = centre[i] + scale * (centre[i] - xold[i])
            if variant == "clamp_order":
                if v > ub[i]:
                    counts["clamp_upper"] += 1
                    v = ub[i]
                if v < lb[i]:
                    counts["clamp_lower"] += 1
                    v = lb[i]
            else:
                if v < lb[i]:
                    counts["clamp_lower"] += 1
                    v = lb[i]
                if v > ub[i]:
                    counts["clamp_upper"] += 1
                    v = ub[i]
            out.append(v)
        if not (all(close(out[i], centre[i]) for i in range(n)) or all(close(out[i], xold[i]) for i in range(n))):
            counts["rf_ok"] += 1
            return out
        counts["rf_coincides"] += 1
        state["status"] = XTOL_REACHED
        raise _Stop

    try:
        # -------------------------------------------------------- start
        state["phase"] = "first"
        value = f(full(start))
        state["minf"] = value
        check(value, start)
        pts, fv = [list(start)], [value]
        for k in range(n):
            at, mag = start[k], abs(step[k])
            p = at + step[k]

            def above(p):
                if p > ub[k]:
                    if ub[k] - at > mag * 0.1:
                        counts["st_above_far"] += 1
                        return ub[k]
                    counts["st_above_near"] += 1
                    return at - mag
                counts["st_plain"] += 1
                return p

            def below(p):
                if p < lb[k]:
                    if at - lb[k] > mag * 0.1:
                        counts["st_below_far"] += 1
                        return lb[k]
                    counts["st_below_near"] += 1
                    p = at + mag
                    if p > ub[k]:
                        counts["st_reversed_outside"] += 1
                        p = 0.5 * ((ub[k] if ub[k] - at > at - lb[k] else lb[k]) + at)
                return p

            p = above(below(p)) if variant == "clamp_order" else below(above(p))
            if close(p, at):
                counts["st_no_move"] += 1
                state["status"] = FAILURE
                raise _Stop
            point = list(start)
            point[k] = p
            pts.append(point)
            fv.append(evaluate(point, "start"))

        # -------------------------------------------------------- loop
        alpha, beta, gamma, delta = 1.0, 0.5, 2.0, 0.5
        order = range(n + 1)
        while True:
            low, high = 0, 0
            for a in order[1:]:
                if variant == "tie_rule":
                    if fv[a] <= fv[low]:
                        low = a
                    if fv[a] > fv[high]:
                        high = a
                else:
                    if fv[a] < fv[low]:
                        low = a
                    if fv[a] >= fv[high]:
                        high = a
            others = [a for a in order if a != high]
            second = others[0]
            for a in others[1:]:
                if fv[a] >= fv[second]:
                    second = a
            fl, fh, fs = fv[low], fv[high], fv[second]
            if any(a != low and fv[a] == fl for a in order):
                counts["tie_low"] += 1
            if any(a != high and fv[a] == fh for a in order):
                counts["tie_high"] += 1

            if math.isfinite(fh):
                if abs(fl - fh) < ftol_rel * (abs(fl) + abs(fh)) * 0.5:
                    counts["ftol_relative"] += 1
                    state["status"] = FTOL_REACHED
                    raise _Stop
                if ftol_rel > 0 and fl == fh:
                    counts["ftol_equal"] += 1
                    state["status"] = FTOL_REACHED
                    raise _Stop
                counts["ftol_go_on"] += 1
            else:
                counts["ftol_not_finite"] += 1

            centre = [0.0] * n
            for a in others:
                for i in range(n):
                    centre[i] += pts[a][i]
            inv = 1.0 / n
            centre = [v * inv for v in centre]

            xr = reflect(centre, alpha, pts[high])
            fr = evaluate(xr, "reflection")
            if fr < fl:
                counts["expand"] += 1
                pts[high] = reflect(centre, gamma, pts[high])
                fv[high] = evaluate(pts[high], "expansion")
                if fv[high] >= fr:
                    counts["expand_rejected"] += 1
                    pts[high], fv[high] = xr, fr
                else:
                    counts["expand_kept"] += 1
            elif fr < fs:
                counts["accept_reflection"] += 1
                pts[high], fv[high] = xr, fr
            else:
                if fh <= fr:
                    counts["contract_inside"] += 1
                    scale = -beta
                else:
                    counts["contract_outside"] += 1
                    scale = beta
                xc = reflect(centre, scale, pts[high])
                fc = evaluate(xc, "contraction")
                if fc < fr and fc < fh:
                    counts["contract_kept"] += 1
                    pts[high], fv[high] = xc, fc
                else:
                    counts["shrink"] += 1
                    for a in order:
                        if a == low:
                            continue
                        pts[a] = reflect(pts[low], -delta, pts[a])
                        fv[a] = evaluate(pts[a], "shrink")
    except _Stop:
        pass
    return done()
