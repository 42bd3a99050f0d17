"""SciPy's differential evolution on the device (csrc/differential_evolution.h, `refine_solve_de_kernel`): the random
stream against `numpy.random.RandomState` and the solver alone against SciPy, bit for bit, on a subset of
tests/_de_cases.py; on the real objective through the public `refine_*` calls, device path against host path
(KPDI_REFINE_DE=host) bit for bit, and by REPLAY - SciPy, seeded alike and fed the device's own objective values in the
device's order, must ask for exactly the device's points and return the device's result."""

import warnings

import numpy as np
import pytest
import scipy.optimize

import _de_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kikuchipy_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ the random stream and the solver alone
@pytest.mark.parametrize("k", dc.GPU_PROGRAMS)
def test_draws_are_random_states(ctx, k):
    seed, rows = dc.PROGRAMS[k]
    got = ctx.mt19937_selftest(seed, dc.program_array(rows))
    want = dc.program_want(seed, rows)
    assert got.dtype == np.uint64 and np.array_equal(got, want), np.flatnonzero(got != want)[:5]


def test_the_subset_covers_what_the_issue_asks():
    cases = [dc.CASES[i] for i in dc.GPU_CASES]
    assert {1, 6} <= {len(c[1][0]) for c in cases}
    assert {c[2].get("updating", "immediate") for c in cases} == {"immediate", "deferred"}
    assert any(c[3].get("redraws") for c in cases) and any(dc.members(c) == dc.DE_POP_MAX for c in cases)


@pytest.mark.parametrize("case", dc.GPU_CASES)
def test_de_matches_scipy_bit_for_bit(ctx, case):
    kind, (lower, upper), kw, _ = dc.CASES[case]
    want, maxiter = dc.want(case)
    got = ctx.de_selftest(kind, lower, upper, dc.members(dc.CASES[case]), maxiter, kw.get("tol", 0.01), kw.get("atol", 0),
                          dc.mutation_pair(kw.get("mutation", (0.5, 1))), kw.get("recombination", 0.7),
                          int(kw.get("init", "latinhypercube") == "random"),
                          int(kw.get("updating", "immediate") == "deferred"), kw["seed"])
    assert (got[1], got[2], got[3]) == (want.nfev, want.nit, int(want.success)), (got, want)
    assert dc.same_bits(got[4:], want.x), (got[4:], want.x)
    assert dc.same_bits(got[0], want.fun), (got[0], want.fun)


def test_refusals(ctx):
    from kikuchipy_amd import _lib

    lower, upper = [0.0] * 3, [1.0] * 3
    for bad, match in ((dict(members=4), "5..256 members"), (dict(members=257), "5..256 members"),
                       (dict(maxiter=-1), "maxiter"), (dict(mutation=2.0), "mutation"), (dict(mutation=(1.0, 0.5)), "mutation"),
                       (dict(init=2), "init"), (dict(updating=2), "updating"), (dict(tol=float("nan")), "NaN")):
        with pytest.raises(_lib.KpdiError, match=match):
            ctx.de_selftest(1, lower, upper, **dict(dict(members=9, maxiter=2), **bad))
    with pytest.raises(_lib.KpdiError, match="bounds must be finite"):
        ctx.de_selftest(1, lower, [1.0, np.inf, 1.0], 9, 2)
    with pytest.raises(_lib.KpdiError, match="lower bounds is greater"):
        ctx.de_selftest(1, upper, lower, 9, 2)
    with pytest.raises(_lib.KpdiError, match="at most 256 entries"):
        ctx.mt19937_selftest(1, [(3, 257, 0)])


# ------------------------------------------------------------------ the real objective
DE = dict(seed=7, popsize=3, maxiter=8)


@pytest.fixture(scope="module")
def inputs():
    """A small Lambert master pattern, a 6 x 8 detector with a signal mask (41 kept pixels: no multiple of anything),
    three patterns - the last one constant, whose centred pattern is zero and whose objective is NaN at every point
    (0 / 0: never accepted, never converged, ends by maxiter) - starts a degree off and one pseudo-symmetry operator
    (two starts per pattern)."""
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


def refine(inputs, mode, **method_kwargs):
    """The public call of `mode`: (scores, num_evals, rotations | None, PCs | None, pseudo-symmetry index | None)."""
    s, det, mp, rot0, mask, op = inputs
    kw = dict(signal_mask=mask, method="differential_evolution", method_kwargs=method_kwargs, verbose=False)
    if mode == "ori":
        res = s.refine_orientation(rot0, det, mp, pseudo_symmetry_ops=op, trust_region=[2, 2, 2], **kw)
        return res.scores, res.num_evals, res.rotations, None, res.pseudo_symmetry_index
    if mode == "pc":
        scores, new_det, num_evals = s.refine_projection_center(rot0, det, mp, trust_region=[0.02] * 3, **kw)
        return scores, num_evals, None, new_det.pc, None
    res, new_det = s.refine_orientation_projection_center(rot0, det, mp, pseudo_symmetry_ops=op,
                                                          trust_region=[2, 2, 2, 0.02, 0.02, 0.02], **kw)
    return res.scores, res.num_evals, res.rotations, new_det.pc, res.pseudo_symmetry_index


@pytest.fixture
def calls(monkeypatch):
    """Counts the host's objective calls and the device solves."""
    from kikuchipy_amd import _lib

    count = dict(objective=0, de=0)

    def counted(name, original):
        def call(self, *args, **kwargs):
            count[name] += 1
            return original(self, *args, **kwargs)
        return call

    monkeypatch.setattr(_lib.Context, "refine_objective", counted("objective", _lib.Context.refine_objective))
    monkeypatch.setattr(_lib.Context, "refine_solve_de", counted("de", _lib.Context.refine_solve_de))
    return count


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.shape(a) == np.shape(b) and dc.same_bits(np.asarray(a, dtype=np.float64).ravel(),
                                                       np.asarray(b, dtype=np.float64).ravel())


@pytest.mark.parametrize("polish", [False, True])
@pytest.mark.parametrize("updating", ["immediate", "deferred"])
@pytest.mark.parametrize("mode", ["ori", "pc", "ori_pc"])
def test_device_path_equals_host_path(inputs, monkeypatch, calls, mode, updating, polish):
    kw = dict(DE, updating=updating) if polish else dict(DE, updating=updating, polish=False)
    monkeypatch.delenv("KPDI_REFINE_DE", raising=False)
    device = refine(inputs, mode, **kw)
    assert calls["de"] == 1 and (calls["objective"] > 0) == polish, calls   # polish=False: no objective call from the host
    made = calls["objective"]
    monkeypatch.setenv("KPDI_REFINE_DE", "host")
    host = refine(inputs, mode, **kw)
    assert calls["de"] == 1 and calls["objective"] > made
    for name, a, b in zip(("scores", "num_evals", "rotations", "pc", "pseudo_symmetry_index"), device, host):
        assert same(a, b), (name, a, b)
    scores, num_evals = device[0], device[1]
    assert np.isnan(scores[2]) and np.all(scores[:2] > 0.5), scores   # the constant pattern; refinements, not noise
    members = max(5, 3 * (6 if mode == "ori_pc" else 3))
    assert np.all(num_evals >= members * 2) and (polish or np.all(num_evals <= members * 9))


@pytest.mark.parametrize("updating", [0, 1])
@pytest.mark.parametrize("mode", ["ori", "ori_pc"])
def test_device_walks_scipys_path_on_its_own_objective_values(ctx, inputs, mode, updating):
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing import _refinement as rf

    s, det, mp, rot0, mask, op = inputs
    ctx.set_master_pattern(*rf._master_pattern_data(mp, None))
    ctx.refine_set_patterns(np.asarray(s.data), mask, False, det.detector_to_sample)
    assert ctx._ref_k == 41
    starts = np.stack([rot0, rf.quaternion_multiply(op[0], rot0)], axis=1)
    euler, pcs = rf.euler_from_rotation(starts), np.tile(det.pc_flattened, (3, 2, 1)).astype(np.float64)
    if mode == "ori":
        code, x0, fixed, tr = _lib.REFINE_ORI, euler, pcs, np.deg2rad([2, 2, 2])
    else:
        code, x0, fixed, tr = _lib.REFINE_ORI_PC, np.concatenate([euler, pcs], axis=2), None, np.array(3 * [np.deg2rad(2)] + 3 * [0.02])
    lower, upper = x0 - tr, x0 + tr
    nvar, members, job, capacity = x0.shape[2], 3 * x0.shape[2], 3, 400   # pattern 1, second start
    seeds = np.arange(11, 17)
    rows, trace, total = ctx.refine_solve_de(code, fixed, lower, upper, members, 8, seeds=seeds, updating=updating,
                                             trace_job=job, trace_capacity=capacity)
    row = rows.reshape(-1, 3 + nvar)[job]
    assert total == row[1] and members * 2 <= total <= members * 9 and trace.shape == (total, nvar + 1)
    asked = [0]

    def replayed(x):
        i = asked[0]
        assert i < total, "SciPy asks for more evaluations than the device made"
        assert dc.same_bits(x, trace[i, :nvar]), (i, x, trace[i, :nvar])
        asked[0] += 1
        return trace[i, nvar]

    bounds = list(zip(lower.reshape(-1, nvar)[job], upper.reshape(-1, nvar)[job]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = scipy.optimize.differential_evolution(replayed, bounds, seed=int(seeds[job]), popsize=3, maxiter=8,
                                                     polish=False, updating=("immediate", "deferred")[updating])
    assert asked[0] == total == want.nfev and row[2] == want.nit
    assert dc.same_bits(row[3:], want.x) and dc.same_bits(row[0], want.fun)
    assert 1 - row[0] > 0.5
    # the trace changes nothing, and every job has its own stream
    assert np.array_equal(ctx.refine_solve_de(code, fixed, lower, upper, members, 8, seeds=seeds, updating=updating), rows,
                          equal_nan=True)
    assert not np.array_equal(rows[0, 0], rows[0, 1])


def test_seed_none_twice(inputs, monkeypatch, calls):
    """Not reproducible, as in SciPy: both results are valid, and they are not required to be equal."""
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing import _refinement as rf

    s, det, mp, rot0, mask, op = inputs
    monkeypatch.delenv("KPDI_REFINE_DE", raising=False)
    c = _lib.Context(0)
    try:
        c.set_master_pattern(*rf._master_pattern_data(mp, None))
        c.refine_set_patterns(np.asarray(s.data)[:2], mask, False, det.detector_to_sample)
        x0, pcs = rf.euler_from_rotation(rot0[:2]), np.tile(det.pc_flattened, (2, 1)).astype(np.float64)
        start_scores = 1 - c.refine_objective(_lib.REFINE_ORI, [0, 1], x0, pcs)
    finally:
        c.close()
    lower, upper = rf._bounds("ori", x0, [2, 2, 2])
    s2 = type(s)(np.asarray(s.data)[:2])
    for _ in range(2):
        res = s2.refine_orientation(rot0[:2], det, mp, signal_mask=mask, method="differential_evolution",
                                    trust_region=[2, 2, 2], method_kwargs=dict(polish=False), verbose=False)
        assert np.all(res.euler >= lower - 1e-12) and np.all(res.euler <= upper + 1e-12)
        assert np.all(res.scores >= start_scores - 1e-12), (res.scores, start_scores)
    assert calls["de"] == 2 and calls["objective"] == 1


def test_what_the_device_does_not_hold_goes_through_the_host(inputs, calls, monkeypatch):
    monkeypatch.delenv("KPDI_REFINE_DE", raising=False)
    for kw in (dict(popsize=86), dict(strategy="rand1bin", popsize=2)):   # 258 members: above the cap
        scores, num_evals = refine(inputs, "ori", seed=3, maxiter=1, polish=False, **kw)[:2]
        assert calls["de"] == 0 and calls["objective"] > 0
        assert np.all(scores[:2] > 0.5) and np.all(num_evals == 2 * max(5, 3 * kw["popsize"]))


def test_navigation_mask_and_deferred_computation(inputs, calls, monkeypatch):
    from kikuchipy_amd.indexing import compute_refine_orientation_results

    s, det, mp, rot0, mask, op = inputs
    monkeypatch.delenv("KPDI_REFINE_DE", raising=False)
    kw = dict(signal_mask=mask, method="differential_evolution", trust_region=[2, 2, 2], verbose=False,
              method_kwargs=dict(DE, polish=False))
    whole = s.refine_orientation(rot0, det, mp, **kw)
    nav = np.array([False, True, False])
    later = s.refine_orientation(rot0, det, mp, navigation_mask=nav, compute=False, **kw)
    assert calls["de"] == 1
    part = compute_refine_orientation_results(later)
    assert calls["de"] == 2 and calls["objective"] == 0
    # seed=k: every job starts from RandomState(k), so a point's result does not depend on which others are refined
    assert same(part.scores, whole.scores[[0, 2]]) and same(part.rotations, whole.rotations[[0, 2]])
