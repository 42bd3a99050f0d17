"""The refinement case tables of tests/_refine_cases.py without a GPU: the float64 restatement of the objective agrees
with the oracle (its formula in float64 to 1e-11, its float32 sums within what they can be off by), the predicted prepared
patterns agree with the oracle's within the float32 pairwise-sum tolerances of tests/test_gpu_refinement.py, the tables
hold every dtype, length, shape, mask, PC and Euler set they are meant to, and every named wrong variant of the
restatement leaves the tolerance on some case - so tests/test_gpu_refine_kernels.py would notice a kernel wrong in that
way."""
import numpy as np
import pytest

import _refine_cases as R
from oracle import kpdi_oracle as ko


@pytest.fixture(scope="module")
def geometries():
    return {g.name: R.build_geometry(g.name) for g in R.GEOMETRIES}


@pytest.fixture(scope="module")
def preps():
    return {c.name: R.build_prep(c.name) for c in R.PREP_CASES + R.EDGE_CASES}


# ---- the objective ------------------------------------------------------------------------------------------------------
def oracle_objective(b, mode, e, i):
    """The oracle's own objective (float32 sums) for evaluation e on pattern i, called as the reference's solvers call it."""
    nrows, ncols = b.geom.shape
    pat, sqn = ko.prepare_refinement_pattern(b.raw[i][b.keep], False)
    keep = b.keep.ravel()
    if mode == "ori":
        dc = ko.direction_cosines_fixed_pc(ko.gnomonic_bounds(b.geom.shape, e.pc), e.pc[2], nrows, ncols, R.OM, keep)
        return ko.refinement_objective(e.eu, "ori", pat, sqn, *b.mp, direction_cosines=dc)
    kw = dict(signal_mask_keep=keep, nrows=nrows, ncols=ncols, om_detector_to_sample=R.OM)
    if mode == "pc":
        return ko.refinement_objective(e.pc, "pc", pat, sqn, *b.mp, rotation=e.q, **kw)
    return ko.refinement_objective(np.concatenate([e.eu, e.pc]), "ori_pc", pat, sqn, *b.mp, **kw)


def oracle_objective64(b, e, i):
    """The oracle's functions in the reference's order - direction cosines, projection to float32, NCC of the centred
    patterns - with the NCC evaluated on float64 copies: its formula (centre, then sum) at full precision."""
    nrows, ncols = b.geom.shape
    dc = ko.direction_cosines_fixed_pc(ko.gnomonic_bounds(b.geom.shape, e.pc), e.pc[2], nrows, ncols, R.OM, b.keep.ravel())
    sim = ko.project_patterns(e.q, dc, *b.mp, False, 0, 1, np.float32)[0]
    assert sim.dtype == np.float32
    return 1 - ko.ncc_exp_centered(b.pat[i].astype(np.float64), sim.astype(np.float64), b.sqn[i])


def float32_sum_bound(sim32, pat, sqn):
    """What the oracle's float32 arithmetic may move its objective by, first order, u = 2^-24: every centred simulated
    value is off by d_c <= u (|sim_c| + |mean|) + (the float32 pairwise mean's L u mean|sim|), every float32 pairwise sum
    of n terms by (L + 1) u sum|terms| with L = ceil(log2 n) + 1 (products included), the squared norm likewise."""
    u, k = 2.0**-24, sim32.size
    L = int(np.ceil(np.log2(k))) + 1
    sim, p = sim32.astype(np.float64), pat.astype(np.float64)
    m = sim.mean()
    c = sim - m
    d = u * (np.abs(sim) + abs(m)) + L * u * np.abs(sim).mean()
    var = (c * c).sum()
    den = np.sqrt(sqn * var)
    ncc = abs((p * c).sum()) / den
    return ((np.abs(p) * d).sum() + (L + 1) * u * np.abs(p * c).sum()) / den + ncc * ((L + 1) * u + (np.abs(c) * d).sum() / var)


def uncentred_term(e, pat, sqn):
    """mean(sim) * sum(pat) / sqrt(sqn * var): what `refine_objective` leaves out when it takes sum(pat * sim) for
    sum(pat * (sim - mean)).  The prepared pattern is centred with a float32 mean, so its sum is k times that mean's
    rounding error and not 0."""
    sim = e.sim32.astype(np.float64)
    var = ((sim - sim.mean()) ** 2).sum()
    return sim.mean() * pat.astype(np.float64).sum() / np.sqrt(sqn * var)


def test_the_restatement_agrees_with_the_oracle(geometries):
    """Every geometry case, PC, Euler set and pattern against the oracle, twice.

    First the oracle's own functions with its NCC formula (centre the simulated pattern, then sum) on float64 copies of
    its float32 values.  The restatement follows the kernel, which sums pat * sim without centring sim; the two differ
    by `uncentred_term` and by nothing else, to 1e-11.  That term is 1e-9 to 1e-8 on ordinary cases and reaches 7.7e-6
    (3.6 times the tolerance) on 1x257 with the PC outside, where the simulated pattern is nearly constant; it is above
    the tolerance on 65 of the 768 cases.  It is a property of the kernel's formula, recorded in DESIGN.md, and the
    kernel is held to the restatement of what it computes.

    Then `ko.refinement_objective` itself, in every mode, as the reference's solvers call it.  It sums in float32:
    one rounding of a total moves it by |NCC| 6e-8, while the restatement's tolerance shrinks to 1e-8 where pattern and
    simulation match (a stationary point of the NCC in the simulated values).  So with the uncentred term taken out,
    the float32 oracle still lies outside the tolerance alone on 120 of the 768 cases, the worst at 7.4 times it
    (1.4e-7 against 1.9e-8); it lies inside the tolerance plus the bound on its own float32 rounding,
    `float32_sum_bound`, on every case, which is what is asserted."""
    worst64, worst, over, at, tols, terms = 0.0, 0.0, 0, None, [], []
    for name, b in geometries.items():
        for e in b.evals:
            for i in range(R.N_PATTERNS):
                tols.append(e.tol[i])
                r = uncentred_term(e, b.pat[i], b.sqn[i])
                terms.append(abs(r) / e.tol[i])
                worst64 = max(worst64, abs(oracle_objective64(b, e, i) - e.f[i] - r))
                own = float32_sum_bound(e.sim32, b.pat[i], b.sqn[i])
                for mode in R.MODES:
                    d = abs(oracle_objective(b, mode, e, i) - e.f[i] - r)
                    over += d > e.tol[i]
                    if d / (e.tol[i] + own) > worst:
                        worst, at = d / (e.tol[i] + own), (name, e.pc_name, e.eu_name, i, mode, d, e.tol[i], own)
    print(f"float64 oracle formula: worst difference {worst64:.1e}; uncentred term above the tolerance on "
          f"{sum(t > 1 for t in terms)} of {len(terms)}, at most {max(terms):.2f} of it; float32 oracle: {over} of "
          f"{3 * len(tols)} outside the tolerance alone, worst share of tolerance + float32 bound {worst:.3f} at {at}; "
          f"tolerances {min(tols):.1e} .. {np.median(tols):.1e} .. {max(tols):.1e}")
    assert worst64 <= 1e-11
    assert worst <= 1.0, (worst, at)
    assert 5e-9 < min(tols) and np.median(tols) < 1e-7 and max(tols) < 1e-4


def test_the_geometry_table_holds_what_it_should(geometries):
    shapes = {g.shape for g in R.GEOMETRIES}
    assert {(5, 7), (7, 5), (16, 16), (1, 257), (12, 20), (3, 3)} <= shapes
    assert {g.mask for g in R.GEOMETRIES} >= {"none", "circular", "checkerboard", "row+last", "one"}
    assert {g.master for g in R.GEOMETRIES} == {"odd", "even"}
    assert R.master("odd")[0].shape == (41, 41) and R.master("even")[0].shape == (40, 40)
    for kind in ("odd", "even"):
        up, lo = R.master(kind)
        assert up.dtype == lo.dtype == np.float32 and not np.array_equal(up, lo)
    assert geometries["16x16-one-masked"].k == 255 and geometries["16x16"].k == 256 and geometries["1x257"].k == 257
    assert sorted(b.k for b in geometries.values())[0] == 8
    assert any(b.k % 64 and b.k % 2 for b in geometries.values())  # odd k: pattern rows at odd float offsets
    # no detector angle is zero; detector -> sample is a rotation
    assert np.allclose(R.OM @ R.OM.T, np.eye(3), atol=1e-15) and (np.abs(R.OM) > 1e-3).sum() >= 8
    # PCs: outside the detector, close to it; Euler sets: Phi = 0, Phi near pi, the sign flip of rotation_from_euler
    assert any(not 0 <= pc[0] <= 1 and not 0 <= pc[1] <= 1 for pc in R.PCS.values())
    assert min(pc[2] for pc in R.PCS.values()) <= 0.15
    phis = [eu[1] for eu in R.EULERS.values()]
    assert 0.0 in phis and any(0 < np.pi - p < 2e-3 for p in phis)
    assert any(np.cos(0.5 * eu[1]) * np.cos(0.5 * (eu[0] + eu[2])) < 0 for eu in R.EULERS.values())
    for name, b in geometries.items():
        assert len(b.evals) == len(R.PCS) * len(R.EULERS) and b.k >= 8
        assert b.raw.dtype == np.uint8 and b.raw.shape == (R.N_PATTERNS,) + b.geom.shape
        assert not np.array_equal(b.raw[0], b.raw[1]) and not np.array_equal(b.raw[1], b.raw[2])
        for e in b.evals:
            assert e.min_abs_z > 1e-9 and e.s2_over_var <= 1e6
            if (e.pc_name, e.eu_name) in R.TWO_HEMISPHERES:
                assert e.share >= 0.1, (name, e.pc_name, e.eu_name, e.share)
        assert sum(e.share >= 0.3 for e in b.evals) >= 2, name
    assert sorted(set(R.PATTERN_INDEX)) == [0, 1, 2] and list(R.PATTERN_INDEX) != sorted(R.PATTERN_INDEX)
    assert len(R.PATTERN_INDEX) > len(set(R.PATTERN_INDEX))
    # the transposed pair: the same kept pixels, transposed
    a, t = geometries["12x20-circular"], geometries["20x12-circular-T"]
    assert np.array_equal(a.keep.T, t.keep) and a.k == t.k


@pytest.mark.parametrize("fault", R.FAULTS)
def test_a_wrong_restatement_leaves_the_tolerance(fault, geometries):
    caught = set()
    for name, b in geometries.items():
        for e in b.evals:
            for i in range(R.N_PATTERNS):
                f, _ = R.objective64(b.geom.shape, b.keep, e.q, e.pc, b.mp, b.pat[i], b.sqn[i], fault)
                if not abs(f - e.f[i]) <= e.tol[i]:
                    caught.add((name, e.pc_name, e.eu_name))
    assert caught, fault
    names = {c[0] for c in caught}
    off_square = {g.name for g in R.GEOMETRIES if g.shape[0] != g.shape[1]}
    if fault == "hemispheres swapped":  # wherever both hemispheres are in view
        assert {(g.name,) + pair for g in R.GEOMETRIES for pair in R.TWO_HEMISPHERES} <= caught
    elif fault == "aspect = nrows / ncols":  # every detector that is not square, and no square one
        assert names == off_square
    elif fault == "no half-pixel offset":
        assert names == set(geometries)
    elif fault == "row and column swapped in the mask map":  # (a map of all pixels of a square detector is symmetric)
        assert off_square <= names and "16x16-one-masked" in names
    else:
        assert off_square - {"1x257", "1x257-checkerboard"} <= names  # (one row: the stride never matters)


def test_the_transposed_detector_is_another_case(geometries):
    """The same pixel values and the same kept pixels on a 20 x 12 detector: every objective moves by at least a
    thousand times what the two tolerances allow together."""
    a, t = geometries["12x20-circular"], geometries["20x12-circular-T"]
    assert np.array_equal(a.raw.transpose(0, 2, 1), t.raw)
    assert np.array_equal(np.sort(a.pat, axis=1), np.sort(t.pat, axis=1)) and np.array_equal(a.sqn, t.sqn)
    for ea, et in zip(a.evals, t.evals):
        assert (np.abs(ea.f - et.f) > 1e3 * (ea.tol + et.tol)).all(), (ea.pc_name, ea.eu_name)


# ---- the preparation ----------------------------------------------------------------------------------------------------
def test_the_prediction_agrees_with_the_oracle(preps):
    """tests/test_gpu_refinement.py allows 1e-4 on a prepared uint8 pattern (values to 255), 1e-6 on a rescaled one
    (values to 1) and 1e-6 relative on the squared norm: what the float32 pairwise mean and sum of the reference are off
    by.  The same here, the first scaled to the largest value of the pattern."""
    for name, b in preps.items():
        c = b.case
        keep = np.ones(c.shape, bool) if b.mask_out is None else ~b.mask_out
        for i in range(R.N_PATTERNS):
            with np.errstate(all="ignore"):
                pat, sqn = ko.prepare_refinement_pattern(b.raw[i][keep], c.rescale)
                top = 1.0 if c.rescale else np.abs(b.raw[i][keep].astype(np.float64)).max() / 255
            if not np.isfinite(b.want_pat[i]).all():
                assert np.array_equal(np.isnan(pat), np.isnan(b.want_pat[i])) and np.isnan(sqn) and np.isnan(b.want_sqn[i]), (name, i)
                ok = ~np.isnan(pat)
                assert np.array_equal(pat[ok], b.want_pat[i][ok]), (name, i)
                continue
            atol = 1e-6 if c.rescale else 1e-4 * max(top, 1e-2)
            assert pat.dtype == np.float32 and np.abs(pat - b.want_pat[i]).max() <= atol, (name, i, np.abs(pat - b.want_pat[i]).max(), atol)
            if b.want_sqn[i] == 0:  # a constant pattern: the float32 mean of the reference need not be the constant itself
                assert 0 <= sqn <= c.k * atol**2, (name, i, sqn)
            else:
                assert np.isclose(sqn, b.want_sqn[i], rtol=1e-6, atol=0), (name, i, sqn, b.want_sqn[i])


def test_the_prep_matrix_is_complete(preps):
    cells = {(c.dtype, c.rescale, c.masked, c.k) for c in R.PREP_CASES}
    assert cells == {(np.dtype(d), r, m, k) for d in R.PREP_DTYPES for r in (False, True) for m in (False, True) for k in R.PREP_K}
    assert len(R.PREP_CASES) == 9 * 2 * 2 * 7 and set(R.PREP_K) == {8, 63, 64, 255, 256, 257, 1000}
    for c in R.PREP_CASES:
        b = preps[c.name]
        assert b.raw.dtype == c.dtype and b.raw.shape == (R.N_PATTERNS,) + c.shape and c.shape[0] != c.shape[1]
        keep = np.ones(c.shape, bool) if b.mask_out is None else ~b.mask_out
        assert keep.sum() == c.k and b.want_pat.shape == (R.N_PATTERNS, c.k) and (b.mask_out is not None) == c.masked
        kept = b.raw[:, keep]
        for i in range(R.N_PATTERNS):
            assert not R.order_complaints(kept[i], c.rescale), c.name
        assert np.isfinite(b.want_pat).all() and (b.want_sqn > 0).all()
        if c.masked:  # what the mask drops would be seen: extremes of the type, NaN among the floats
            out = b.raw[:, ~keep]
            assert np.isnan(out).any() if c.dtype.kind == "f" else (out.max() == np.iinfo(c.dtype).max and out.min() == np.iinfo(c.dtype).min)
            assert not (np.diff(np.flatnonzero(keep)) == 1).all()
        if c.dtype.kind == "i":
            assert (kept < 0).mean() > 0.2
        if c.dtype in (np.int32, np.uint32):  # values the cast to float32 rounds
            assert (np.abs(kept.astype(np.int64)) > 2**24).mean() > 0.9
            assert (kept.astype(np.float32).astype(np.int64) != kept.astype(np.int64)).any()
        if c.dtype == np.float64:
            assert (kept.astype(np.float32).astype(np.float64) != kept).mean() > 0.9


def test_the_edge_rows_are_what_the_reference_defines(preps):
    seen = set()
    for c in R.EDGE_CASES:
        b = preps[c.name]
        keep = ~b.mask_out
        pat, sqn, kind = b.want_pat[1], b.want_sqn[1], c.recipe[0]
        kept = b.raw[1][keep]
        if kind == "constant":
            assert (kept == kept[0]).all() and not (b.raw[1][~keep] == kept[0]).any()
            if c.rescale:  # 0 / 0
                assert np.isnan(pat).all() and np.isnan(sqn)
            else:
                assert not pat.any() and sqn == 0 and not np.signbit(sqn)
        else:
            assert (~np.isfinite(kept)).sum() == 1 and not np.isfinite(kept[c.recipe[2]])
            assert np.isnan(sqn) and not np.isfinite(pat).any()
            if kind == "nan" or c.rescale:
                assert np.isnan(pat).all()
            else:  # an infinite mean: the pixel itself inf - inf, every other one finite - inf
                at = np.flatnonzero(np.isnan(pat))
                assert at.tolist() == [c.recipe[2]] and (np.delete(pat, at) == -c.recipe[1]).all()
            if kind == "nan" and c.rescale:  # fminf / fmaxf skip the NaN, np.min / np.max do not: same end
                lo, hi = np.fmin.reduce(kept.astype(np.float32)), np.fmax.reduce(kept.astype(np.float32))
                with np.errstate(invalid="ignore"):
                    v = (kept.astype(np.float32) - lo) / np.float32(hi - lo) * np.float32(2) + np.float32(-1)
                assert np.isfinite(lo) and np.isfinite(hi) and np.isnan(v).sum() == 1
                assert np.isnan(np.float32(v.astype(np.float64).sum() / v.size))
        for i in (0, 2):  # the neighbours of the edge row are ordinary patterns
            assert np.isfinite(b.want_pat[i]).all() and b.want_sqn[i] > 0
        seen.add((kind, c.dtype.name, c.rescale))
    assert {s for s in seen if s[0] != "constant"} == {(k, d, r) for k in ("nan", "inf", "neginf") for d in ("float32", "float64", "float16")
                                                      for r in (False, True)}
    assert {s[1] for s in seen if s[0] == "constant"} >= {"uint8", "float32", "float64", "uint32"}
