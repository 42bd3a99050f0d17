"""The LN_NELDERMEAD search on the device (csrc/nlopt_simplex.h, `refine_solve_nlopt_kernel`): the search alone
against the host build of the header (and the Python restatement) bit for bit on the cases of
tests/_nlopt_simplex_cases.py; on the real objective against the restatement driven through `ctx.refine_objective`, one
evaluation per call; and through the public `refine_*` calls what the reference's own tests ask of this method
(tests/test_indexing/test_ebsd_refinement.py:560-640, :1030-1080 of the reference).  NLopt itself is not compared with.

The refinement fixture (tests/golden/refinement.npz) holds four 60 x 60 Ni patterns with their starting orientations and
PCs; they are what every test below runs on."""

import numpy as np
import pytest

import _nlopt_simplex_cases as nc
import _nlopt_simplex_restate as restate
import test_host_nlopt_simplex as host
from conftest import load_golden
from oracle import kpdi_oracle as ko

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    return load_golden("refinement.npz")


@pytest.fixture(scope="module")
def master():
    p = load_golden("projection.npz")
    return p["mp_upper"], p["mp_lower"]


@pytest.fixture(scope="module")
def ctx(master):
    from kikuchipy_amd import _lib

    c = _lib.Context(0)
    c.set_master_pattern(*ko.refinement_master_pattern(*master))
    yield c
    c.close()


# ------------------------------------------------------------------ the search alone
@pytest.fixture(scope="module")
def header_rows(tmp_path_factory):
    return host.run_driver(host.build_driver(tmp_path_factory.mktemp("nlopt_simplex_gpu")), nc.CASES)[0]


@pytest.mark.parametrize("case", range(len(nc.CASES)), ids=[c.name for c in nc.CASES])
def test_selftest_matches_the_host_header_bit_for_bit(ctx, header_rows, case):
    c = nc.CASES[case]
    lower, upper = c.lower, c.upper
    if (lower is None) != (upper is None):  # the entry takes both or neither: the missing side is infinite
        lower = [-np.inf] * len(c.x0) if lower is None else lower
        upper = [np.inf] * len(c.x0) if upper is None else upper
    got = ctx.nlopt_simplex_selftest(c.kind, c.x0, lower, upper, c.xstep, c.ftol_rel, c.maxeval)
    status, nevals, minf, x = host.header_result(header_rows[case])
    assert (got[2], got[1]) == (status, nevals), (got, header_rows[case])
    assert nc.same_bits(got[3:], x), (got[3:], x)
    assert nc.same_bits(got[0], minf), (got[0], minf)
    want = nc.want(case)  # and the restatement, which the host test holds the header to
    assert (got[2], got[1]) == (want.status, want.nevals) and nc.same_bits(got[3:], want.x) and nc.same_bits(got[0], want.minf)


def test_refusals(ctx, g):
    from kikuchipy_amd import _lib

    ctx.refine_set_patterns(g["patterns"].reshape(-1, 60, 60), None, False, g["om_detector_to_sample"])
    x0, fixed = g["eu0"][:, None, :], g["pc0"][:, None, :]
    with pytest.raises(_lib.KpdiError, match="ftol_rel > 0 or maxeval > 0"):
        ctx.refine_solve_nlopt(_lib.REFINE_ORI, x0, fixed, ftol_rel=0.0)
    with pytest.raises(_lib.KpdiError, match="ftol_rel > 0 or maxeval > 0"):
        ctx.nlopt_simplex_selftest(1, [1.0, 1.0])
    bad = x0.copy()
    bad[1, 0, 2] = np.nan
    with pytest.raises(_lib.KpdiError, match="starting point is not finite"):
        ctx.refine_solve_nlopt(_lib.REFINE_ORI, bad, fixed)
    with pytest.raises(_lib.KpdiError, match="initial step is not finite"):
        ctx.refine_solve_nlopt(_lib.REFINE_ORI, x0, fixed, xstep=[0.1, np.inf, 0.1])
    with pytest.raises(_lib.KpdiError, match="a bound is NaN"):
        ctx.refine_solve_nlopt(_lib.REFINE_ORI, x0, fixed, x0 - 0.01, bad + 0.01)
    with pytest.raises(_lib.KpdiError, match="xstep must have 3 values"):
        ctx.refine_solve_nlopt(_lib.REFINE_ORI, x0, fixed, xstep=[0.1] * 6)
    with pytest.raises(_lib.KpdiError, match="kind must be within 0..5"):
        ctx.nlopt_simplex_selftest(6, [1.0, 1.0], maxeval=5)
    with pytest.raises(_lib.KpdiError, match="4 patterns were set"):
        ctx.refine_solve_nlopt(_lib.REFINE_ORI, x0[:3], fixed[:3])
    # a start outside its box and a step of zero are results of the search, not refusals of the entry
    rows = ctx.refine_solve_nlopt(_lib.REFINE_ORI, x0, fixed, x0 + 0.01, x0 + 0.02, maxeval=5)
    assert np.all(rows[:, :, 2] == restate.INVALID_ARGS) and np.all(rows[:, :, 1] == 0)
    rows = ctx.refine_solve_nlopt(_lib.REFINE_ORI, x0, fixed, xstep=[0.1, 0.0, 0.1], maxeval=5)
    assert np.all(rows[:, :, 2] == restate.FAILURE) and np.all(rows[:, :, 1] == 2)


# ------------------------------------------------------------------ the real objective, against the restatement
N_COMPARED = 2  # patterns; every evaluation of the restatement is one call into the device
STEPS = {"ori": [0.1] * 3, "pc": [0.05] * 3, "ori_pc": [0.1] * 3 + [0.05] * 3}   # the tutorial's initial steps
REGION = {"ori": np.deg2rad([5.0] * 3), "pc": np.array([0.05] * 3),
          "ori_pc": np.concatenate([np.deg2rad([5.0] * 3), [0.05] * 3])}        # the tutorial's trust region


def solve_inputs(g, mode, starts=1):
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing._refinement import rotation_from_euler

    eu = g["eu0"][:N_COMPARED, None, :]
    pc = g["pc0"][:N_COMPARED, None, :]
    if starts == 2:  # the second start: the first displaced by a degree about every Euler angle
        eu = np.concatenate([eu, eu + np.deg2rad(1.0)], axis=1)
        pc = np.repeat(pc, 2, axis=1)
    if mode == "ori":
        return _lib.REFINE_ORI, eu, pc
    if mode == "pc":
        return _lib.REFINE_PC, pc, rotation_from_euler(eu)
    return _lib.REFINE_ORI_PC, np.concatenate([eu, pc], axis=2), None


def assert_same_search(rows, want_rows):
    """The standard tests/test_gpu_powell.py holds the device Powell to against a host-driven run of the same search
    (`assert_same_refinement` there: scores within 2e-4, evaluation counts within a quarter, variables within 2e-3).
    That file does not establish that the in-kernel objective and `kpdi_refine_objective` agree to the bit - its replay
    feeds the host the KERNEL's values - so bit equality is printed here, not asserted."""
    rows, want_rows = rows.reshape(-1, rows.shape[-1]), want_rows.reshape(-1, rows.shape[-1])
    same = np.array_equal(rows, want_rows)
    print("bit for bit:", same, "| max |dscore|", np.abs(rows[:, 0] - want_rows[:, 0]).max(), "| nevals", rows[:, 1],
          want_rows[:, 1], "| status", rows[:, 2], want_rows[:, 2], "| max |dx|", np.abs(rows[:, 3:] - want_rows[:, 3:]).max())
    assert np.abs(rows[:, 0] - want_rows[:, 0]).max() < 2e-4
    assert np.all(np.abs(rows[:, 1] - want_rows[:, 1]) <= 0.25 * want_rows[:, 1])
    assert np.abs(rows[:, 3:] - want_rows[:, 3:]).max() < 2e-3


def restated_rows(ctx, code, x0, fixed, lower, upper, xstep, ftol_rel, maxeval):
    out = np.empty(x0.shape[:2] + (3 + x0.shape[2],))
    for p in range(x0.shape[0]):
        for s in range(x0.shape[1]):
            fx = None if fixed is None else fixed[p, s][None]
            r = restate.optimize(lambda x: float(ctx.refine_objective(code, [p], np.asarray(x)[None], fx)[0]), x0[p, s],
                                 None if lower is None else lower[p, s], None if upper is None else upper[p, s], xstep,
                                 ftol_rel, maxeval)
            out[p, s, 0], out[p, s, 1], out[p, s, 2], out[p, s, 3:] = r.minf, r.nevals, r.status, r.x
    return out


@pytest.mark.parametrize("bounded", [False, True], ids=["free", "trust_region"])
@pytest.mark.parametrize("mode", ["ori", "pc", "ori_pc"])
def test_solver_matches_the_restatement_on_the_real_objective(ctx, g, mode, bounded):
    ctx.refine_set_patterns(g["patterns"].reshape(-1, 60, 60)[:N_COMPARED], None, False, g["om_detector_to_sample"])
    code, x0, fixed = solve_inputs(g, mode)
    lower, upper = (x0 - REGION[mode], x0 + REGION[mode]) if bounded else (None, None)
    rows = ctx.refine_solve_nlopt(code, x0, fixed, lower, upper, STEPS[mode], ftol_rel=1e-3, maxeval=150)
    want_rows = restated_rows(ctx, code, x0, fixed, lower, upper, STEPS[mode], 1e-3, 150)
    assert_same_search(rows, want_rows)
    assert np.all(np.isin(rows[:, :, 2], (restate.FTOL_REACHED, restate.MAXEVAL_REACHED))) and np.all(rows[:, :, 1] <= 150)
    start = ctx.refine_objective(code, np.arange(N_COMPARED), x0[:, 0], None if fixed is None else fixed[:, 0])
    assert np.all(rows[:, 0, 0] <= start)  # the lowest value seen, the start's included
    if bounded:
        assert np.all(rows[:, :, 3:] >= lower) and np.all(rows[:, :, 3:] <= upper)


def test_solver_matches_the_restatement_with_two_starts(ctx, g):
    """Each (pattern, start) is a search of its own, with its own evaluation count; no initial step: the default one."""
    ctx.refine_set_patterns(g["patterns"].reshape(-1, 60, 60)[:N_COMPARED], None, False, g["om_detector_to_sample"])
    code, x0, fixed = solve_inputs(g, "ori", starts=2)
    lower, upper = x0 - REGION["ori"], x0 + REGION["ori"]
    rows = ctx.refine_solve_nlopt(code, x0, fixed, lower, upper, None, ftol_rel=1e-3, maxeval=120)
    assert rows.shape == (N_COMPARED, 2, 6)
    assert_same_search(rows, restated_rows(ctx, code, x0, fixed, lower, upper, None, 1e-3, 120))


# ------------------------------------------------------------------ what the reference's tests ask of this method
@pytest.fixture(scope="module")
def api_inputs(g, master):
    import kikuchipy_amd as ka
    from kikuchipy_amd.indexing._refinement import rotation_from_euler

    mp = ka.EBSDMasterPattern(np.stack(master), phase_name="ni")
    pats = g["patterns"].reshape(2, 2, 60, 60)
    det = ka.EBSDDetector(shape=(60, 60), pc=g["pc0"].reshape(2, 2, 3), sample_tilt=70)
    rot0 = rotation_from_euler(g["eu0"]).reshape(2, 2, 4)
    return ka.EBSD(pats), det, mp, rot0


@pytest.fixture
def device_path(monkeypatch):
    monkeypatch.delenv("KPDI_REFINE_NLOPT", raising=False)


def test_refine_orientation_improves_the_scores(api_inputs, device_path, capsys):
    s, det, mp, rot0 = api_inputs
    mask = ~ko.circular_window((60, 60)).astype(bool)
    kw = dict(signal_mask=mask, method="LN_NELDERMEAD", trust_region=[2, 2, 2])
    start = s.refine_orientation(rot0, det, mp, maxeval=1, verbose=False, **kw)   # one evaluation: the start itself
    assert np.all(start.num_evals == 1)
    res = s.refine_orientation(rot0, det, mp, **kw)
    assert "Method: LN_NELDERMEAD (local) from NLopt, restated on the GPU" in capsys.readouterr().out
    assert res.scores.mean() > start.scores.mean() and np.all(res.scores >= start.scores)
    assert res.scores.shape == (4,) and res.rotations.shape == (4, 4) and res.scores.mean() > 0.8
    capped = s.refine_orientation(rot0, det, mp, maxeval=20, rtol=1e-3, verbose=False, **kw)
    assert capped.num_evals.max() <= 20


def test_refine_projection_center_stays_in_the_trust_region(api_inputs, device_path):
    s, det, mp, rot0 = api_inputs
    scores, new_det, num_evals = s.refine_projection_center(rot0, det, mp, method="LN_NELDERMEAD", initial_step=0.01,
                                                            rtol=1e-2, maxeval=40, trust_region=[0.02] * 3, verbose=False)
    assert num_evals.max() <= 40 and scores.size == 4
    assert new_det.pc.shape == det.pc.shape and not np.allclose(new_det.pc, det.pc)
    assert np.abs(new_det.pc - det.pc).max() <= 0.02 + 1e-12


def test_pseudo_symmetry_index_selects_the_displaced_start(api_inputs, device_path):
    from kikuchipy_amd.indexing._refinement import quaternion_multiply

    s, det, mp, rot0 = api_inputs
    half = np.deg2rad(30) / 2
    ops = np.array([[np.cos(half), 0, 0, np.sin(half)], [np.cos(half), 0, 0, -np.sin(half)]])  # 30 degrees about +-z
    displaced = rot0.copy()
    displaced[0, 0] = quaternion_multiply(ops[0], rot0[0, 0])  # so that the second operator (the inverse) is the best match
    kw = dict(method="LN_NELDERMEAD", trust_region=[2, 2, 2], verbose=False)
    start = s.refine_orientation(displaced, det, mp, maxeval=1, **kw)
    res = s.refine_orientation(displaced, det, mp, pseudo_symmetry_ops=ops, **kw)
    assert res.scores.mean() > start.scores.mean()
    assert np.array_equal(res.pseudo_symmetry_index, [2, 0, 0, 0])


def test_the_tutorials_call_direct_and_deferred(api_inputs, device_path):
    from kikuchipy_amd.indexing import _refinement as rf

    s, det, mp, rot0 = api_inputs
    kw = dict(method="LN_NELDERMEAD", trust_region=[5, 5, 5, 0.05, 0.05, 0.05], rtol=1e-3, initial_step=[0.1, 0.05],
              verbose=False)
    start, _ = s.refine_orientation_projection_center(rot0, det, mp, maxeval=1, **kw)
    res, new_det = s.refine_orientation_projection_center(rot0, det, mp, **kw)
    assert res.scores.mean() > start.scores.mean() and res.scores.mean() > 0.8
    assert np.abs(new_det.pc - det.pc).max() <= 0.05 + 1e-12 and new_det.pc.shape == det.pc.shape
    deferred = s.refine_orientation_projection_center(rot0, det, mp, compute=False, **kw)
    assert isinstance(deferred, rf.DeferredRefinement)
    later, later_det = rf.compute_refine_orientation_projection_center_results(deferred, det, None, mp)
    assert np.array_equal(later.scores, res.scores) and np.array_equal(later.num_evals, res.num_evals)
    assert np.array_equal(later.rotations, res.rotations) and np.array_equal(later_det.pc, new_det.pc)
    assert deferred.compute().shape == (4, 8)


def test_results_do_not_depend_on_the_split(g, master, api_inputs, device_path):
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing import _refinement as rf

    s, det, mp, rot0 = api_inputs
    pats = g["patterns"].reshape(2, 2, 60, 60)
    kw = dict(method="LN_NELDERMEAD", trust_region=[5, 5, 5, 0.05, 0.05, 0.05], rtol=1e-3, initial_step=[0.1, 0.05],
              maxeval=120, verbose=False)
    with _lib.Context(0) as a, _lib.Context(0) as b:
        whole, whole_det = rf.refine("ori_pc", pats, rot0, det, mp, context=a, **kw)
        split, split_det = rf.refine("ori_pc", pats, rot0, det, mp, contexts=[a, b], **kw)
    assert np.array_equal(whole.scores, split.scores) and np.array_equal(whole.num_evals, split.num_evals)
    assert np.array_equal(whole.euler, split.euler) and np.array_equal(whole_det.pc, split_det.pc)
