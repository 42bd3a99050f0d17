"""SciPy's Powell on the device (csrc/powell.h, `refine_solve_powell_kernel`): the optimiser alone against SciPy bit for
bit on the analytic cases of tests/_powell_cases.py; on the real objective by REPLAY - SciPy, fed the device's own
objective values in the device's order, must ask for exactly the device's points and return the device's result; and
through the public `refine_*` calls against the host-driven path (KPDI_REFINE_POWELL=host)."""

import warnings

import numpy as np
import pytest
import scipy.optimize

import _powell_cases as pc
from conftest import load_golden
from oracle import kpdi_oracle as ko

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return load_golden("refinement.npz")


@pytest.fixture(scope="module")
def ctx():
    from kikuchipy_amd import _lib

    c = _lib.Context(0)
    p = load_golden("projection.npz")
    c.set_master_pattern(*ko.refinement_master_pattern(p["mp_upper"], p["mp_lower"]))
    yield c
    c.close()


# ------------------------------------------------------------------ the optimiser alone
@pytest.mark.parametrize("case", range(len(pc.CASES)))
def test_powell_matches_scipy_bit_for_bit(ctx, case):
    kind, x0, bounds, opt, _ = pc.CASES[case]
    want = pc.want(case)
    got = ctx.powell_selftest(kind, x0, *(bounds or (None, None)), xtol=opt.get("xtol", 1e-4), ftol=opt.get("ftol", 1e-4),
                              maxiter=opt.get("maxiter", 0), maxfev=opt.get("maxfev", 0))
    assert (got[1], got[2], got[3]) == (want.nfev, want.nit, want.status), (got, want)
    assert pc.same_bits(got[4:], want.x), (got[4:], want.x)
    assert pc.same_bits(got[0], want.fun), (got[0], want.fun)


# ------------------------------------------------------------------ the real objective, by replay
TRACE_CAPACITY = 4000
REPLAY = ["ori", "ori_bounded", "pc_tutorial", "ori_pc_bounded", "ori_masked", "ori_maxfev", "ori_two_starts"]


@pytest.mark.parametrize("config", REPLAY)
def test_device_walks_scipys_path_on_its_own_objective_values(ctx, g, config):
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing._refinement import rotation_from_euler

    eu0, pc0 = g["eu0"], g["pc0"]
    mask = ~ko.circular_window((60, 60)).astype(bool) if config == "ori_masked" else None
    ctx.refine_set_patterns(g["patterns"].reshape(-1, 60, 60), mask, False, g["om_detector_to_sample"])
    if mask is not None:
        assert ctx._ref_k == 2819  # not a multiple of the 256 threads
    options, job = {}, 0
    lower = upper = None
    if config == "pc_tutorial":
        mode, x0, fixed = _lib.REFINE_PC, pc0[:, None, :], rotation_from_euler(eu0)[:, None, :]
        lower, upper = x0 - 0.02, x0 + 0.02
        options = dict(xtol=1e-3, ftol=1e-3)
    elif config == "ori_pc_bounded":
        mode, x0, fixed = _lib.REFINE_ORI_PC, np.concatenate([eu0, pc0], axis=1)[:, None, :], None
        tr = np.array(3 * [np.deg2rad(2)] + 3 * [0.02])
        lower, upper = x0 - tr, x0 + tr
    else:
        mode, x0, fixed = _lib.REFINE_ORI, eu0[:, None, :], pc0[:, None, :]
        if config == "ori_bounded":
            lower, upper = x0 - np.deg2rad(2), x0 + np.deg2rad(2)
        elif config == "ori_maxfev":
            options = dict(maxfev=30)
        elif config == "ori_two_starts":
            x0 = np.concatenate([x0, x0 + np.deg2rad([0.7, -0.4, 0.5])], axis=1)
            fixed = np.repeat(fixed, 2, axis=1)
            job = 1  # pattern 0, second start
    rows, trace, total = ctx.refine_solve_powell(mode, x0, fixed, lower, upper, xtol=options.get("xtol", 1e-4),
                                                 ftol=options.get("ftol", 1e-4), maxfev=options.get("maxfev", 0),
                                                 trace_job=job, trace_capacity=TRACE_CAPACITY)
    nvar = x0.shape[2]
    row = rows.reshape(-1, 3 + nvar)[job]
    assert total == row[1] and total <= TRACE_CAPACITY and trace.shape == (total, nvar + 1)
    if config == "ori_maxfev":
        assert total == 30
    calls = [0]

    def replayed(x):
        i = calls[0]
        assert i < total, "SciPy asks for more evaluations than the device made"
        assert pc.same_bits(x, trace[i, :nvar]), (i, x, trace[i, :nvar])
        calls[0] += 1
        return trace[i, nvar]

    start = x0.reshape(-1, nvar)[job]
    bounds = None if lower is None else list(zip(lower.reshape(-1, nvar)[job], upper.reshape(-1, nvar)[job]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = scipy.optimize.minimize(replayed, start, method="Powell", bounds=bounds, options=options)
    assert calls[0] == total == want.nfev
    assert pc.same_bits(row[3:], want.x), (row[3:], want.x)
    assert pc.same_bits(row[0], want.fun) and row[2] == want.nit
    assert 1 - row[0] > 0.5  # a refinement, not a walk through noise


def test_trace_beyond_its_capacity_is_counted_not_stored(ctx, g):
    from kikuchipy_amd import _lib

    ctx.refine_set_patterns(g["patterns"].reshape(-1, 60, 60), None, False, g["om_detector_to_sample"])
    x0, fixed = g["eu0"][:, None, :], g["pc0"][:, None, :]
    rows, trace, total = ctx.refine_solve_powell(_lib.REFINE_ORI, x0, fixed, trace_job=3, trace_capacity=4000)
    short_rows, short, short_total = ctx.refine_solve_powell(_lib.REFINE_ORI, x0, fixed, trace_job=3, trace_capacity=7)
    assert np.array_equal(rows, short_rows) and short_total == total > 7
    assert short.shape == (7, 4) and np.array_equal(short, trace[:7])
    assert np.array_equal(ctx.refine_solve_powell(_lib.REFINE_ORI, x0, fixed), rows)  # the trace changes nothing


# ------------------------------------------------------------------ public interface: device path against host path
@pytest.fixture(scope="module")
def api_inputs(g):
    import kikuchipy_amd as ka
    from kikuchipy_amd.indexing._refinement import rotation_from_euler

    p = load_golden("projection.npz")
    mp = ka.EBSDMasterPattern(np.stack([p["mp_upper"], p["mp_lower"]]), phase_name="ni")
    pats = g["patterns"].reshape(2, 2, 60, 60)
    det = ka.EBSDDetector(shape=(60, 60), pc=g["pc0"].reshape(2, 2, 3), sample_tilt=70)
    rot0 = rotation_from_euler(g["eu0"]).reshape(2, 2, 4)
    return ka.EBSD(pats), det, mp, rot0


@pytest.fixture
def objective_calls(monkeypatch):
    from kikuchipy_amd import _lib

    calls = [0]
    original = _lib.Context.refine_objective

    def counted(self, *args, **kwargs):
        calls[0] += 1
        return original(self, *args, **kwargs)

    monkeypatch.setattr(_lib.Context, "refine_objective", counted)
    return calls


def both_paths(call, monkeypatch, capsys, objective_calls):
    """`call()` on the device path, then on the host path: the two results and the (identical) message."""
    monkeypatch.delenv("KPDI_REFINE_POWELL", raising=False)
    objective_calls[0] = 0
    capsys.readouterr()
    device = call()
    said = capsys.readouterr().out
    assert objective_calls[0] == 0, "the device path called the objective from the host"
    monkeypatch.setenv("KPDI_REFINE_POWELL", "host")
    host = call()
    said_host = capsys.readouterr().out
    assert objective_calls[0] > 0

    def information(text):
        return text[:text.index("Refining")]

    assert "Method: Powell (local) from SciPy" in said and information(said) == information(said_host)
    return device, host


def assert_same_refinement(scores, scores_host, evals, evals_host, euler=None, euler_host=None, pcs=None, pcs_host=None):
    # the tolerances the project uses between two evaluations of this objective (tests/test_gpu_refinement.py:363-364)
    print("scores", scores, scores_host, "evaluations", evals, evals_host)
    assert np.abs(scores - scores_host).max() < 2e-4
    assert np.all(np.abs(evals.astype(int) - evals_host.astype(int)) <= 0.25 * evals_host)
    if euler is not None:
        assert np.abs(euler - euler_host).max() < 2e-3
    if pcs is not None:
        assert np.abs(pcs - pcs_host).max() < 2e-3


@pytest.mark.parametrize("trust_region", [None, [2, 2, 2]])
def test_refine_orientation_device_against_host(api_inputs, monkeypatch, capsys, objective_calls, trust_region):
    s, det, mp, rot0 = api_inputs
    dev, host = both_paths(lambda: s.refine_orientation(rot0, det, mp, method_kwargs=dict(method="Powell"),
                                                        trust_region=trust_region), monkeypatch, capsys, objective_calls)
    assert_same_refinement(dev.scores, host.scores, dev.num_evals, host.num_evals, dev.euler, host.euler)
    assert dev.scores.mean() > 0.8


def test_refine_projection_center_device_against_host(api_inputs, monkeypatch, capsys, objective_calls):
    """The call of the reference's pattern-matching tutorial."""
    s, det, mp, rot0 = api_inputs
    dev, host = both_paths(lambda: s.refine_projection_center(rot0, det, mp, method_kwargs=dict(method="Powell", tol=1e-3),
                                                              trust_region=[0.02] * 3), monkeypatch, capsys, objective_calls)
    assert_same_refinement(dev[0], host[0], dev[2], host[2], pcs=dev[1].pc, pcs_host=host[1].pc)
    assert np.abs(dev[1].pc - det.pc).max() <= 0.02 + 1e-12 and not np.allclose(dev[1].pc, det.pc)


def test_refine_orientation_projection_center_device_against_host(api_inputs, monkeypatch, capsys, objective_calls):
    s, det, mp, rot0 = api_inputs
    dev, host = both_paths(lambda: s.refine_orientation_projection_center(
        rot0, det, mp, method_kwargs=dict(method="Powell"), trust_region=[2, 2, 2, 0.02, 0.02, 0.02]),
        monkeypatch, capsys, objective_calls)
    assert_same_refinement(dev[0].scores, host[0].scores, dev[0].num_evals, host[0].num_evals, dev[0].euler, host[0].euler,
                           dev[1].pc, host[1].pc)


def test_pseudo_symmetry_device_against_host(api_inputs, monkeypatch, capsys, objective_calls):
    from kikuchipy_amd.indexing._refinement import quaternion_multiply

    s, det, mp, rot0 = api_inputs
    op = np.array([[np.cos(np.deg2rad(10)), 0, 0, np.sin(np.deg2rad(10))]])
    powell = dict(method="Powell")
    dev, host = both_paths(lambda: s.refine_orientation(rot0, det, mp, pseudo_symmetry_ops=op, method_kwargs=powell),
                           monkeypatch, capsys, objective_calls)
    assert np.abs(dev.scores - host.scores).max() < 2e-4
    # the two starts on their own: where their scores are further apart than twice the tolerance, the winner is the same
    monkeypatch.delenv("KPDI_REFINE_POWELL", raising=False)
    first = s.refine_orientation(rot0, det, mp, method_kwargs=powell, verbose=False)
    second = s.refine_orientation(quaternion_multiply(op[0], rot0), det, mp, method_kwargs=powell, verbose=False)
    clear = np.abs(first.scores - second.scores) > 4e-4
    assert clear.any()
    assert np.array_equal(dev.pseudo_symmetry_index[clear], host.pseudo_symmetry_index[clear])
    assert np.array_equal(dev.pseudo_symmetry_index[clear], (second.scores > first.scores)[clear].astype(int))


# ------------------------------------------------------------------ refusals
def test_refusals(ctx, g):
    from kikuchipy_amd import _lib

    ctx.refine_set_patterns(g["patterns"].reshape(-1, 60, 60), None, False, g["om_detector_to_sample"])
    x0, fixed = g["eu0"][:, None, :], g["pc0"][:, None, :]
    upper = x0 + 0.01
    for bad in (np.inf, np.nan):
        upper_bad = upper.copy()
        upper_bad[2, 0, 1] = bad
        with pytest.raises(_lib.KpdiError, match="bounds must be finite"):
            ctx.refine_solve_powell(_lib.REFINE_ORI, x0, fixed, x0 - 0.01, upper_bad)
    lower_bad = x0 - 0.01
    lower_bad[0, 0, 0] = -np.inf
    with pytest.raises(_lib.KpdiError, match="bounds must be finite"):
        ctx.refine_solve_powell(_lib.REFINE_ORI, x0, fixed, lower_bad, upper)
    with pytest.raises(_lib.KpdiError, match="lower bounds is greater"):
        ctx.refine_solve_powell(_lib.REFINE_ORI, x0, fixed, upper, x0 - 0.01)
    with pytest.raises(_lib.KpdiError, match="bounds must be finite"):
        ctx.powell_selftest(1, [2.0, 1.0, 0.5], [0.5, 0.0, 0.0], [2.05, np.inf, 0.6])
    with pytest.raises(_lib.KpdiError, match=r"x0 must have shape \(n_patterns, n_starts, 6\)"):
        ctx.refine_solve_powell(_lib.REFINE_ORI_PC, x0, None)
    with pytest.raises(_lib.KpdiError, match="trace"):
        ctx.refine_solve_powell(_lib.REFINE_ORI, x0, fixed, trace_job=4, trace_capacity=10)
    with pytest.raises(_lib.KpdiError, match="4 patterns were set"):
        ctx.refine_solve_powell(_lib.REFINE_ORI, x0[:3], fixed[:3])
