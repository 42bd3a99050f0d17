"""refine_prep_kernel and refine_objective of csrc/refine.hip on their own, through the C ABI, on the tables of
tests/_refine_cases.py (tests/test_host_refine_cases.py shows what those tables can see).

Preparation: all nine dtypes x rescale off and on x mask off and on x k in {8, 63, 64, 255, 256, 257, 1000}, three
patterns each on detectors that are not square, and the constant / NaN / +-inf rows: prepared pattern and squared norm
BIT FOR BIT what `prep64` predicts (any NaN for any NaN).

Objective: sixteen geometries (shapes off the square, one row, masks, two different hemispheres, odd and even master
pattern) x four PCs x four Euler sets x three modes on patterns indexed out of order: |kernel - objective64| within the
tolerance the restatement derives for each value.  Measured on MI355X: the largest |kernel - objective64| / tolerance
over the 3 x 1024 values is 5.4e-8 (9.6e-14 against 1.8e-6, 1x257-checkerboard); no float32 cast fell the other way.

In-kernel objective: `refine_objective` is inlined into the three device solvers; what they record (every evaluation of
a Powell trace, the final value of each solver) against kpdi_refine_objective at the same point, within twice the
tolerance.  Measured on MI355X: all 306 values (270 traced, 36 final) bit-equal to the objective kernel's.

And one complete Nelder-Mead refinement of twelve 12 x 20 patterns under a circular mask, both hemispheres in view,
against the oracle's SciPy loop within the limits of test_many_patterns_against_the_scipy_loop."""
import numpy as np
import pytest

import _refine_cases as R
from kikuchipy_amd import _lib
from oracle import kpdi_oracle as ko

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


# ---- preparation --------------------------------------------------------------------------------------------------------
def prepared(ctx, b):
    ctx.set_master_pattern(*R.master("odd"))  # (the prepared pattern does not depend on it)
    ctx.refine_set_patterns(b.raw, b.mask_out, b.case.rescale, R.OM)
    return ctx.refine_get_prepared()


def prep_complaints(ctx, cases):
    bad = []
    for c in cases:
        b = R.build_prep(c.name)
        pat, sqn = prepared(ctx, b)
        assert pat.shape == b.want_pat.shape and pat.dtype == np.float32 and sqn.dtype == np.float64
        for i in range(R.N_PATTERNS):
            if not R.same_bits(pat[i], b.want_pat[i]):
                at = np.flatnonzero(~((pat[i] == b.want_pat[i]) | (np.isnan(pat[i]) & np.isnan(b.want_pat[i]))))
                bad.append((c.name, i, "pattern", len(at), int(at[0]) if len(at) else None,
                            repr(pat[i][at[:1]]), repr(b.want_pat[i][at[:1]])))
            if not R.same_bits(sqn[i:i + 1], b.want_sqn[i:i + 1]):
                bad.append((c.name, i, "squared norm", repr(sqn[i]), repr(b.want_sqn[i])))
    return bad


@pytest.mark.parametrize("dtype", [np.dtype(d).name for d in R.PREP_DTYPES])
def test_prepared_patterns_bit_for_bit(ctx, dtype):
    cases = [c for c in R.PREP_CASES if c.dtype.name == dtype]
    assert len(cases) == 28
    bad = prep_complaints(ctx, cases)
    assert not bad, (len(bad), bad[:6])


def test_constant_nan_and_infinite_rows(ctx):
    """A constant pattern: zeros and a squared norm of +0, or all NaN under rescale (0 / 0).  One NaN or +-inf among the
    kept pixels: NaN squared norm and no finite pixel (all NaN, but for an infinite pixel without rescale: the mean is
    infinite, so the pixel itself is NaN and every other one -+inf).  The patterns either side stay ordinary."""
    bad = prep_complaints(ctx, R.EDGE_CASES)
    assert not bad, (len(bad), bad[:6])
    b = R.build_prep("edge-constant-uint8-plain")
    pat, sqn = prepared(ctx, b)
    assert not pat[1].any() and sqn[1] == 0 and not np.signbit(sqn[1]) and not np.signbit(pat[1]).any()


# ---- the objective ------------------------------------------------------------------------------------------------------
def load(ctx, b):
    ctx.set_master_pattern(*b.mp)
    ctx.refine_set_patterns(b.raw, b.mask_out, False, R.OM)
    pat, sqn = ctx.refine_get_prepared()
    assert R.same_bits(pat, b.pat) and R.same_bits(sqn, b.sqn), b.geom.name  # what objective64 was given


@pytest.mark.parametrize("mode", list(R.MODES))
def test_objective_against_the_restatement(ctx, mode):
    worst, at, n, bad = 0.0, None, 0, []
    for g in R.GEOMETRIES:
        b = R.build_geometry(g.name)
        load(ctx, b)
        idx, x, fixed, want, tol, labels = R.objective_batch(b, R.MODES[mode])
        got = ctx.refine_objective(R.MODES[mode], idx, x, fixed)
        ratio = np.abs(got - want) / tol
        n += len(got)
        for j in np.flatnonzero(~(ratio <= 1)):
            bad.append((labels[j], got[j], want[j], tol[j]))
        j = int(np.nanargmax(ratio))
        if ratio[j] > worst:
            worst, at = float(ratio[j]), (labels[j], got[j], want[j], tol[j])
    print(f"{mode}: {n} values, largest |kernel - objective64| / tolerance {worst:.2e} at {at}")
    assert not bad, (len(bad), bad[:6])


def test_the_same_pixels_on_a_transposed_detector(ctx):
    """A 12 x 20 pattern and its transpose under the transposed mask: the kernel gives two different sets of values,
    each its own restatement's (a swapped row and column, an inverted aspect or a wrong stride in the mask map would
    make one of them the other's, or neither)."""
    got = {}
    for name in ("12x20-circular", "20x12-circular-T"):
        b = R.build_geometry(name)
        load(ctx, b)
        idx, x, fixed, want, tol, labels = R.objective_batch(b, R.ORI_PC)
        got[name] = ctx.refine_objective(R.ORI_PC, idx, x, fixed)
        assert (np.abs(got[name] - want) <= tol).all(), name
        got[name + " tol"] = tol
    a, t = got["12x20-circular"], got["20x12-circular-T"]
    assert (np.abs(a - t) > 1e3 * (got["12x20-circular tol"] + got["20x12-circular-T tol"])).all()


# ---- the objective inside the solvers -----------------------------------------------------------------------------------
def tolerance_at(b, mode, x, fixed, i):
    if mode == R.PC:
        q, pc = fixed, x
    else:
        q, pc = ko.rotation_from_euler(*x[:3]), (fixed if mode == R.ORI else x[3:])
    return R.objective64(b.geom.shape, b.keep, q, pc, b.mp, b.pat[i], b.sqn[i])


@pytest.mark.parametrize("mode", list(R.MODES))
def test_the_solvers_evaluate_the_objective_kernels_objective(ctx, mode):
    """12x20-circular, both hemispheres in view, three patterns from half a degree and 0.005 off their Euler angles and
    PC, inside bounds.  Every evaluation Powell traced for job 0 (half the pixels in either hemisphere) and the final
    value of every job of the three solvers, against kpdi_refine_objective at the same x: one operation compiled into
    four kernels, which may differ by contraction only - twice the tolerance of the point."""
    code = R.MODES[mode]
    b = R.build_geometry("12x20-circular")
    load(ctx, b)
    assert min(e.share for e in b.evals if (e.pc_name, e.eu_name) == ("mid", "plain")) >= 0.3
    eu = np.array([R.EULERS[n] for n in ("plain", "flip", "PhiPi")]) + np.deg2rad(0.5) * np.array([[1, -1, 1], [-1, 1, 1], [1, 1, -1]])
    pc = np.tile(R.PCS["mid"], (3, 1)) + 0.005 * np.array([[1, -1, 1], [-1, -1, 1], [1, 1, -1]])
    half_eu, half_pc = np.full(3, np.deg2rad(2.0)), np.full(3, 0.03)
    if code == R.ORI:
        x0, fixed, half = eu, pc, half_eu
    elif code == R.PC:
        x0, fixed, half = pc, np.array([ko.rotation_from_euler(*e) for e in eu]), half_pc
    else:
        x0, fixed, half = np.concatenate([eu, pc], axis=1), None, np.concatenate([half_eu, half_pc])
    nvar = x0.shape[1]
    x0, lo, hi = x0[:, None, :], (x0 - half)[:, None, :], (x0 + half)[:, None, :]
    fx = None if fixed is None else fixed[:, None, :]

    def check(what, idx, x, f):
        kernel = ctx.refine_objective(code, idx, x, None if fixed is None else fixed[idx])
        same = 0
        for j in range(len(idx)):
            want, tol = tolerance_at(b, code, x[j], None if fixed is None else fixed[idx[j]], idx[j])
            assert abs(f[j] - kernel[j]) <= 2 * tol, (what, j, f[j], kernel[j], tol)
            assert abs(kernel[j] - want) <= tol, (what, j, kernel[j], want, tol)
            same += int(f[j] == kernel[j])
        print(f"{mode} {what}: {same} of {len(idx)} in-kernel values bit-equal to the objective kernel's, largest difference "
              f"{np.abs(np.asarray(f) - kernel).max():.2e}")
        return same

    res, trace, total = ctx.refine_solve_powell(code, x0, fx, lo, hi, maxfev=90, trace_job=0, trace_capacity=256)
    assert total == len(trace) >= 20 and np.isfinite(trace).all()
    check("Powell trace", np.zeros(len(trace), int), trace[:, :nvar], trace[:, nvar])
    jobs = np.arange(3)
    check("Powell result", jobs, res[:, 0, 3:], res[:, 0, 0])
    res = ctx.refine_solve(code, x0, fx, lo, hi, maxfev=60)
    check("Nelder-Mead result", jobs, res[:, 0, 3:], res[:, 0, 0])
    res = ctx.refine_solve_nlopt(code, x0, fx, lo, hi, maxeval=60)
    check("LN_NELDERMEAD result", jobs, res[:, 0, 3:], res[:, 0, 0])


# ---- one complete solve off the square ----------------------------------------------------------------------------------
def test_a_refinement_on_a_masked_12x20_detector_against_the_scipy_loop(ctx):
    pats, keep, pc, eu, eu0, mp = R.solve_inputs()
    n = len(pats)
    ctx.set_master_pattern(*mp)
    ctx.refine_set_patterns(pats, ~keep, False, R.OM)
    res = ctx.refine_solve(R.ORI, eu0[:, None, :], np.tile(pc, (n, 1, 1)))[:, 0]
    dc = ko.direction_cosines_fixed_pc(ko.gnomonic_bounds(keep.shape, pc), pc[2], *keep.shape, R.OM, keep.ravel())
    for i in range(n):
        want = ko.refine_solver(pats[i][keep], "ori", eu0[i], *mp, False, direction_cosines=dc)
        print(i, f"score {1 - res[i, 0]:.6f} vs {want[0]:.6f}, |dx| {np.abs(res[i, 3:6] - np.array(want[2:5])).max():.2e}, "
                 f"nfev {int(res[i, 1])} vs {want[1]}")
        assert abs((1 - res[i, 0]) - want[0]) < 2e-4, (i, 1 - res[i, 0], want[0])
        assert np.abs(res[i, 3:6] - np.array(want[2:5])).max() < 2e-3, (i, res[i, 3:6], want[2:5])
    assert np.median(np.abs(res[:, 3:6] - eu)) < np.median(np.abs(eu0 - eu)) / 3
