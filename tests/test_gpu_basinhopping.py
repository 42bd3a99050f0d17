"""SciPy's basinhopping around Nelder-Mead on the device (csrc/basinhopping.h, `refine_solve_basinhopping_kernel`): the
solver alone against SciPy, bit for bit, on a subset of tests/_basinhopping_cases.py; on the real objective through the
public `refine_*` calls, device path against host path (KPDI_REFINE_BASINHOPPING=host) bit for bit, and by REPLAY -
SciPy, seeded alike and fed the device's own objective values in the device's order, must ask for exactly the device's
points and return the device's result; with the host's objective call taken away the public call still succeeds."""

import warnings

import numpy as np
import pytest
import scipy.optimize

import _basinhopping_cases as bc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kikuchipy_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------ the solver alone
def test_the_subset_covers_what_the_issue_asks():
    cases = [bc.CASES[i] for i in bc.GPU_CASES]
    assert {1, 6} <= {len(c[1]) for c in cases}
    assert any(c[2].get("T") == 0 for c in cases) and any(c[2].get("interval") == 2 for c in cases)
    assert any(c[3].get("early") for c in cases) and any(c[3].get("mixed") for c in cases)
    assert any(c[2]["niter"] == 0 for c in cases) and any(c[0] == 4 for c in cases)


@pytest.mark.parametrize("case", bc.GPU_CASES)
def test_basinhopping_matches_scipy_bit_for_bit(ctx, case):
    kind, x0, kw, _ = bc.CASES[case]
    want, hops = bc.want(case)
    assert bc.margin_ok(hops)
    xatol, fatol, maxiter, maxfev = bc.quench_options(bc.CASES[case])
    got = ctx.basinhopping_selftest(kind, x0, kw["niter"], kw.get("T", 1.0), kw.get("stepsize", 0.5), kw.get("interval", 50),
                                    kw.get("niter_success"), kw.get("target_accept_rate", 0.5),
                                    kw.get("stepwise_factor", 0.9), xatol, fatol, maxiter, maxfev, kw["seed"])
    assert tuple(got[1:5]) == (want.nfev, want.nit, int(want.success), want.minimization_failures), (got, want)
    assert bc.same_bits(got[5:], want.x), (got[5:], want.x)
    assert bc.same_bits(got[0], want.fun), (got[0], want.fun)


def test_refusals(ctx):
    from kikuchipy_amd import _lib

    nan = float("nan")
    for bad, match in ((dict(interval=0), "interval"), (dict(interval=-2), "interval"), (dict(niter=-1), "niter"),
                       (dict(target_accept_rate=0.0), "target_accept_rate"), (dict(target_accept_rate=1.0), "target_accept_rate"),
                       (dict(stepwise_factor=0.0), "stepwise_factor"), (dict(stepwise_factor=1.5), "stepwise_factor"),
                       (dict(T=nan), "NaN"), (dict(stepsize=nan), "NaN"), (dict(target_accept_rate=nan), "NaN"),
                       (dict(stepwise_factor=nan), "NaN"), (dict(xatol=nan), "NaN"), (dict(fatol=nan), "NaN"),
                       (dict(stepsize=float("inf")), "stepsize")):
        with pytest.raises(_lib.KpdiError, match=match):
            ctx.basinhopping_selftest(1, [1.0, 1.0, 1.0], **dict(dict(niter=2), **bad))
    with pytest.raises(_lib.KpdiError, match="kind"):
        ctx.basinhopping_selftest(5, [1.0, 1.0, 1.0], niter=2)
    with pytest.raises(_lib.KpdiError, match="nvar"):
        ctx.basinhopping_selftest(1, [1.0] * 7, niter=2)


# ------------------------------------------------------------------ the real objective
@pytest.fixture(scope="module")
def inputs():
    return bc.real_inputs()


def refine(inputs, mode, **method_kwargs):
    """The public call of `mode`: (scores, num_evals, rotations | None, PCs | None, pseudo-symmetry index | None)."""
    s, det, mp, rot0, mask, op = inputs
    kw = dict(signal_mask=mask, method="basinhopping", method_kwargs=method_kwargs, verbose=False)
    if mode == "ori":
        res = s.refine_orientation(rot0, det, mp, pseudo_symmetry_ops=op, **kw)
        return res.scores, res.num_evals, res.rotations, None, res.pseudo_symmetry_index
    if mode == "pc":
        scores, new_det, num_evals = s.refine_projection_center(rot0, det, mp, **kw)
        return scores, num_evals, None, new_det.pc, None
    res, new_det = s.refine_orientation_projection_center(rot0, det, mp, pseudo_symmetry_ops=op, **kw)
    return res.scores, res.num_evals, res.rotations, new_det.pc, res.pseudo_symmetry_index


@pytest.fixture
def calls(monkeypatch):
    """Counts the host's objective calls and the device solves."""
    from kikuchipy_amd import _lib

    count = dict(objective=0, bh=0)

    def counted(name, original):
        def call(self, *args, **kwargs):
            count[name] += 1
            return original(self, *args, **kwargs)
        return call

    monkeypatch.setattr(_lib.Context, "refine_objective", counted("objective", _lib.Context.refine_objective))
    monkeypatch.setattr(_lib.Context, "refine_solve_basinhopping",
                        counted("bh", _lib.Context.refine_solve_basinhopping))
    return count


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.shape(a) == np.shape(b) and bc.same_bits(np.asarray(a, dtype=np.float64).ravel(),
                                                       np.asarray(b, dtype=np.float64).ravel())


@pytest.mark.parametrize("mode", ["ori", "pc", "ori_pc"])
def test_device_path_equals_host_path(inputs, monkeypatch, calls, mode):
    assert bc.BH["niter"] <= 6 and bc.BH["minimizer_kwargs"]["options"]["maxfev"] <= 60
    monkeypatch.delenv("KPDI_REFINE_BASINHOPPING", raising=False)
    device = refine(inputs, mode, **bc.BH)
    assert calls == dict(objective=0, bh=1), calls   # no objective call from the host
    monkeypatch.setenv("KPDI_REFINE_BASINHOPPING", "host")
    host = refine(inputs, mode, **bc.BH)
    assert calls["bh"] == 1 and calls["objective"] > 0
    for name, a, b in zip(("scores", "num_evals", "rotations", "pc", "pseudo_symmetry_index"), device, host):
        assert same(a, b), (name, a, b)
    scores, num_evals = device[0], device[1]
    assert np.isnan(scores[2]) and np.all(scores[:2] > 0.5), scores   # the constant pattern; refinements, not noise
    nvar, quenches, maxfev = (6 if mode == "ori_pc" else 3), bc.BH["niter"] + 1, 50
    assert np.all(num_evals >= quenches * (nvar + 1)) and np.all(num_evals <= quenches * maxfev)   # a simplex per quench
    assert num_evals[2] == quenches * maxfev   # NaN everywhere: every quench ends by its budget


@pytest.mark.parametrize("mode", ["ori", "pc", "ori_pc"])
def test_device_walks_scipys_path_on_its_own_objective_values(ctx, inputs, mode):
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing import _refinement as rf

    s, det, mp, rot0, mask, op = inputs
    ctx.set_master_pattern(*rf._master_pattern_data(mp, None))
    ctx.refine_set_patterns(np.asarray(s.data), mask, False, det.detector_to_sample)
    assert ctx._ref_k == 41
    starts = np.stack([rot0, rf.quaternion_multiply(op[0], rot0)], axis=1)
    euler, pcs = rf.euler_from_rotation(starts), np.tile(det.pc_flattened, (3, 2, 1)).astype(np.float64)
    if mode == "ori":
        code, x0, fixed = _lib.REFINE_ORI, euler, pcs
    elif mode == "pc":
        code, x0, fixed = _lib.REFINE_PC, pcs, starts
    else:
        code, x0, fixed = _lib.REFINE_ORI_PC, np.concatenate([euler, pcs], axis=2), None
    nvar, job, capacity = x0.shape[2], 3, 7 * 60   # pattern 1, second start
    seeds = np.arange(11, 17)
    kw = dict(niter=6, T=0.01, stepsize=0.02, interval=2, maxfev=60)
    rows, trace, total = ctx.refine_solve_basinhopping(code, x0, fixed, seeds=seeds, trace_job=job,
                                                       trace_capacity=capacity, **kw)
    row = rows.reshape(-1, 3 + nvar)[job]
    assert total == row[1] and nvar + 1 <= total <= capacity and trace.shape == (total, nvar + 1)
    asked = [0]

    def replayed(x):
        i = asked[0]
        assert i < total, "SciPy asks for more evaluations than the device made"
        assert bc.same_bits(x, trace[i, :nvar]), (i, x, trace[i, :nvar])
        asked[0] += 1
        return trace[i, nvar]

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want, hops = bc.replay(replayed, x0.reshape(-1, nvar)[job], seed=int(seeds[job]), niter=6, T=0.01, stepsize=0.02,
                               interval=2, minimizer_kwargs=dict(method="Nelder-Mead", options=dict(maxfev=60)))
    assert asked[0] == total == want.nfev and row[2] == want.nit
    assert bc.same_bits(row[3:], want.x) and bc.same_bits(row[0], want.fun)
    assert 1 - row[0] > 0.5
    # the trace changes nothing, and every job has its own stream
    assert np.array_equal(ctx.refine_solve_basinhopping(code, x0, fixed, seeds=seeds, **kw), rows, equal_nan=True)
    assert not np.array_equal(rows[0, 0], rows[0, 1])


def test_no_objective_call_from_the_host(inputs, monkeypatch):
    """The whole search runs on the device: the public call succeeds with the host's objective call taken away."""
    from kikuchipy_amd import _lib

    def refused(self, *args, **kwargs):
        raise AssertionError("the host evaluated the objective")

    monkeypatch.delenv("KPDI_REFINE_BASINHOPPING", raising=False)
    monkeypatch.setattr(_lib.Context, "refine_objective", refused)
    scores, num_evals = refine(inputs, "ori", **bc.BH)[:2]
    assert np.all(scores[:2] > 0.5) and np.all(num_evals > 0)


def test_navigation_mask_and_deferred_computation(inputs, calls, monkeypatch):
    from kikuchipy_amd.indexing import compute_refine_orientation_results

    s, det, mp, rot0, mask, op = inputs
    monkeypatch.delenv("KPDI_REFINE_BASINHOPPING", raising=False)
    kw = dict(signal_mask=mask, method="basinhopping", verbose=False, method_kwargs=bc.BH)
    whole = s.refine_orientation(rot0, det, mp, **kw)
    nav = np.array([False, True, False])
    later = s.refine_orientation(rot0, det, mp, navigation_mask=nav, compute=False, **kw)
    assert calls["bh"] == 1
    part = compute_refine_orientation_results(later)
    assert calls["bh"] == 2 and calls["objective"] == 0
    # seed=k: every job starts from RandomState(k), so a point's result does not depend on which others are refined
    assert same(part.scores, whole.scores[[0, 2]]) and same(part.rotations, whole.rotations[[0, 2]])


def test_several_contexts_and_seed_none(inputs, calls, monkeypatch):
    """The `contexts` route splits the points; `seed=None` draws fresh seeds: valid results, not required to be equal."""
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing import _refinement as rf

    s, det, mp, rot0, mask, op = inputs
    monkeypatch.delenv("KPDI_REFINE_BASINHOPPING", raising=False)
    kw = dict(signal_mask=mask, method="basinhopping", verbose=False)
    one = rf.refine("ori", np.asarray(s.data), rot0, det, mp, method_kwargs=bc.BH, **kw)[0]
    a, b = _lib.Context(0), _lib.Context(0)
    try:
        two = rf.refine("ori", np.asarray(s.data), rot0, det, mp, method_kwargs=bc.BH, contexts=[a, b], **kw)[0]
    finally:
        a.close()
        b.close()
    assert calls["bh"] == 3 and calls["objective"] == 0
    assert same(one.scores, two.scores) and same(one.rotations, two.rotations) and same(one.num_evals, two.num_evals)
    fresh = rf.refine("ori", np.asarray(s.data)[:2], rot0[:2], det, mp, method_kwargs=dict(bc.BH, seed=None), **kw)[0]
    assert np.all(fresh.scores > 0.5) and calls["objective"] == 0
