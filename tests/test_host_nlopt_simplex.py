"""The LN_NELDERMEAD search without a GPU: csrc/nlopt_simplex.h compiled with the host compiler and run over
tests/_nlopt_simplex_cases.py against the plain-Python restatement of DESIGN.md section 21 bit for bit, with every named
branch reached by both and three deliberately wrong restatements caught; and the dispatch of
`refine(..., method="LN_NELDERMEAD")` with a stand-in context.  NLopt itself takes no part: it is not installed where
this suite runs."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import _nlopt_simplex_cases as nc
import _nlopt_simplex_restate as restate
from kikuchipy_amd.indexing import _refinement as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The six objectives are csrc/analytic_objectives.h, in the operation order of tests/_nlopt_simplex_cases.py.  One line
# per case on stdin:
#   kind n has_lower has_upper has_xstep ftol_rel maxeval x0[n] [lower[n]] [upper[n]] [xstep[n]]   (floats as C99 hex)
# one line per case out: status nevals minf x[n] (floats as their 64 bits), then "count <name> <hits>" per branch.
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "analytic_objectives.h"
#include "nlopt_simplex.h"

using Analytic = kpdi::AnalyticObjective;

static unsigned long long bits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, 8);
  return u;
}

int main() {
  char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    char *p = line;
    Analytic f;
    f.kind = (int)std::strtol(p, &p, 10);
    f.n = (int)std::strtol(p, &p, 10);
    const int has_lower = (int)std::strtol(p, &p, 10), has_upper = (int)std::strtol(p, &p, 10);
    const int has_step = (int)std::strtol(p, &p, 10);
    const double ftol_rel = std::strtod(p, &p);
    const long long maxeval = std::strtoll(p, &p, 10);
    double x0[6], lo[6], hi[6], step[6];
    if (f.n < 1 || f.n > 6) return 2;
    for (int i = 0; i < f.n; ++i) x0[i] = std::strtod(p, &p);
    if (has_lower) for (int i = 0; i < f.n; ++i) lo[i] = std::strtod(p, &p);
    if (has_upper) for (int i = 0; i < f.n; ++i) hi[i] = std::strtod(p, &p);
    if (has_step) for (int i = 0; i < f.n; ++i) step[i] = std::strtod(p, &p);
    kpdi::NloptSimplex<6, Analytic> ns(f);
    ns.optimize(f.n, x0, has_lower ? lo : nullptr, has_upper ? hi : nullptr, has_step ? step : nullptr, ftol_rel, maxeval);
    std::printf("%d %lld %016llx", ns.status, ns.nevals, bits(ns.minf));
    for (int i = 0; i < f.n; ++i) std::printf(" %016llx", bits(ns.x[i]));
    std::printf("\n");
  }
  for (int b = 0; b < kpdi::NSB_COUNT; ++b)
    std::printf("count %s %lld\n", kpdi::kpdi_nlopt_branch_names[b], kpdi::kpdi_nlopt_count[b]);
  return 0;
}
"""


def case_line(case):
    words = [str(case.kind), str(len(case.x0)), *("0" if a is None else "1" for a in (case.lower, case.upper, case.xstep)),
             float(case.ftol_rel).hex(), str(case.maxeval)]
    for a in (case.x0, case.lower, case.upper, case.xstep):
        if a is not None:
            words += [float(v).hex() for v in a]
    return " ".join(words)


def build_driver(tmp):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp / "nlopt_simplex_driver.cpp", tmp / "nlopt_simplex_driver"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-DKPDI_NLOPT_COUNT", "-I",
                    os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return exe


def run_driver(exe, cases):
    text = "\n".join(case_line(c) for c in cases) + "\n"
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.strip().split("\n")
    rows = [ln.split() for ln in out if not ln.startswith("count ")]
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in out if ln.startswith("count ")}
    assert len(rows) == len(cases)
    return rows, counts


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    return run_driver(build_driver(tmp_path_factory.mktemp("nlopt_simplex")), nc.CASES)


def from_bits(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


def header_result(row):
    return int(row[0]), int(row[1]), from_bits(row[2:3])[0], from_bits(row[3:])


def differs(row, want):
    status, nevals, minf, x = header_result(row)
    return ((status, nevals) != (want.status, want.nevals) or not nc.same_bits(x, want.x)
            or not nc.same_bits(minf, want.minf))


IDS = [c.name for c in nc.CASES]


def test_case_names_are_unique_and_cases_are_small():
    assert len(set(IDS)) == len(IDS)
    for i, c in enumerate(nc.CASES):
        assert 1 <= len(c.x0) <= 6 and nc.want(i).nevals <= 400, c.name


@pytest.mark.parametrize("case", range(len(nc.CASES)), ids=IDS)
def test_restatement_does_what_the_table_says(case):
    """The table's own claims (where the search ends, which branches a row is there for) hold for the restatement."""
    want, expect = nc.want(case), nc.CASES[case].expect
    if "status" in expect:
        assert restate.STATUS_NAMES[want.status] == expect["status"]
    if "nevals" in expect:
        assert want.nevals == expect["nevals"]
    if "phase" in expect:
        assert want.phase == expect["phase"]
    for name in expect.get("hits", ()):
        assert name in restate.BRANCHES and want.counts[name] > 0, name
    assert set(want.counts) <= set(restate.BRANCHES)


@pytest.mark.parametrize("case", range(len(nc.CASES)), ids=IDS)
def test_header_matches_the_restatement_bit_for_bit(driver_output, case):
    status, nevals, minf, x = header_result(driver_output[0][case])
    want = nc.want(case)
    assert (status, nevals) == (want.status, want.nevals), (driver_output[0][case], want)
    assert nc.same_bits(x, want.x), (x, want.x)
    assert nc.same_bits(minf, want.minf), (minf, want.minf)


def test_every_named_branch_is_reached_by_both(driver_output):
    counts = driver_output[1]
    assert sorted(counts) == sorted(restate.BRANCHES)
    total = restate.collections.Counter()
    for i in range(len(nc.CASES)):
        total.update(nc.want(i).counts)
    assert not [name for name in restate.BRANCHES if counts[name] == 0], "not reached by the header"
    assert not [name for name in restate.BRANCHES if total[name] == 0], "not reached by the restatement"
    # the same arms the same number of times: the two walk the same path, not only to the same end
    assert {name: total[name] for name in restate.BRANCHES} == counts


def test_maxeval_lands_on_every_check_position():
    phases = {nc.want(i).phase for i, c in enumerate(nc.CASES) if nc.want(i).status == restate.MAXEVAL_REACHED}
    assert {"first", "start", "reflection", "expansion", "contraction", "shrink"} <= phases


@pytest.mark.parametrize("variant", ["tie_rule", "clamp_order", "check_order"])
def test_a_wrong_restatement_fails_the_table(driver_output, variant):
    caught = [c.name for i, c in enumerate(nc.CASES) if differs(driver_output[0][i], nc.want(i, variant))]
    print(variant, "caught by", caught)
    assert caught


def test_tie_rule_as_stated():
    """Low point: the lower storage index among equals; high point: the higher.  Four equal values at the start and a
    budget of one more evaluation: the reflected point is point 3 mirrored in the centroid of points 0, 1 and 2."""
    seen = []

    def flat(x):
        seen.append(list(x))
        return 1.0

    restate.optimize(flat, [0.0, 0.0, 0.0], xstep=[3.0, 3.0, 3.0], maxeval=5)
    assert seen[4] == [2.0, 2.0, -3.0]


# ------------------------------------------------------------------ the dispatch of `refine`
class _Recorder:
    """Stands in for the engine context of `refine`: records the solver and objective calls."""

    def __init__(self, status=3):
        self.nlopt, self.objective, self.status = [], 0, status

    def set_master_pattern(self, up, lo):
        pass

    def refine_set_patterns(self, pats, signal_mask, rescale, om):
        pass

    def refine_solve_nlopt(self, mode, x0, fixed, lower, upper, xstep, ftol_rel, maxeval):
        self.nlopt.append(dict(mode=mode, n=len(x0), bounded=lower is not None, xstep=xstep, ftol_rel=ftol_rel,
                               maxeval=maxeval))
        out = np.zeros(x0.shape[:2] + (3 + x0.shape[2],))
        out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3:] = 0.25, 77, self.status, x0
        return out

    def refine_objective(self, mode, pattern_index, x, fixed=None):
        self.objective += len(pattern_index)
        return np.array([0.5 + float(np.sum((np.asarray(xx) - 0.1) ** 2)) for xx in x])


@pytest.fixture
def inputs():
    import kikuchipy_amd as ka

    det = ka.EBSDDetector(shape=(6, 6), pc=(0.4, 0.6, 0.5))
    mp = ka.EBSDMasterPattern(np.random.default_rng(0).random((11, 11), dtype=np.float32))
    pats = np.random.default_rng(1).integers(0, 255, (2, 3, 6, 6), dtype=np.uint8)
    rot = np.tile([1.0, 0, 0, 0], (2, 3, 1))
    return pats, rot, det, mp


def test_refine_sends_ln_neldermead_to_the_device(monkeypatch, inputs, capsys):
    """On the parent commit this call raises ImportError: NLopt's Python module is the only way there."""
    monkeypatch.delenv("KPDI_REFINE_NLOPT", raising=False)

    def run(mode="ori", method="LN_NELDERMEAD", contexts=None, verbose=False, **kwargs):
        ctx = _Recorder()
        kw = dict(contexts=contexts(ctx)) if contexts else dict(context=ctx)
        out = rf.refine(mode, *inputs, method=method, verbose=verbose, **kwargs, **kw)
        return ctx, out

    ctx, (res, det) = run(initial_step=0.1, rtol=1e-3, maxeval=50)
    assert ctx.nlopt == [dict(mode=rf.MODES["ori"], n=6, bounded=False, xstep=[0.1, 0.1, 0.1], ftol_rel=1e-3, maxeval=50)]
    assert ctx.objective == 0 and det is None
    assert np.array_equal(res.num_evals, np.full(6, 77)) and np.allclose(res.scores, 0.75)
    ctx, _ = run("pc", method="ln_neldermead", initial_step=[0.05], trust_region=[0.02] * 3)
    assert ctx.nlopt == [dict(mode=rf.MODES["pc"], n=6, bounded=True, xstep=[0.05] * 3, ftol_rel=1e-4, maxeval=0)]
    # the tutorial's call
    ctx, (res, det) = run("ori_pc", initial_step=[0.1, 0.05], rtol=1e-3, trust_region=[5, 5, 5, 0.05, 0.05, 0.05])
    assert ctx.nlopt == [dict(mode=rf.MODES["ori_pc"], n=6, bounded=True, xstep=[0.1] * 3 + [0.05] * 3, ftol_rel=1e-3,
                              maxeval=0)]
    assert det.pc.shape == (2, 3, 3)
    ctx, _ = run("ori_pc", method="Ln_NelderMead")   # no initial step: the search's default step
    assert ctx.nlopt[0]["xstep"] is None and ctx.nlopt[0]["bounded"] is False
    ctx, _ = run(contexts=lambda c: [c, c], initial_step=0.1)   # one call per block of points
    assert [call["n"] for call in ctx.nlopt] == [3, 3] and ctx.objective == 0
    # compute=False: nothing runs until the deferred object is asked
    ctx = _Recorder()
    deferred = rf.refine("ori_pc", *inputs, method="LN_NELDERMEAD", initial_step=[0.1, 0.05], verbose=False, context=ctx,
                         compute=False)
    assert ctx.nlopt == []
    res, det = rf.compute_refine_orientation_projection_center_results(deferred)
    assert len(ctx.nlopt) == 1 and deferred.compute().shape == (6, 8) and res.scores.shape == (6,)


def test_kpdi_refine_nlopt_host_restores_the_host_path(monkeypatch, inputs):
    import importlib.util

    ctx = _Recorder()
    monkeypatch.setenv("KPDI_REFINE_NLOPT", "host")
    if importlib.util.find_spec("nlopt") is None:
        with pytest.raises(ImportError, match="requires the optional dependency 'nlopt'"):
            rf.refine("ori", *inputs, method="LN_NELDERMEAD", initial_step=0.1, context=ctx, verbose=False)
    else:  # NLopt itself on the host, the objective through the context
        rf.refine("ori", *inputs, method="LN_NELDERMEAD", initial_step=0.1, maxeval=5, context=ctx, verbose=False)
        assert ctx.objective == 6 * 5
        ctx.objective = 0
    assert ctx.nlopt == []
    monkeypatch.setenv("KPDI_REFINE_NLOPT", "device")   # anything but "host"
    rf.refine("ori", *inputs, method="LN_NELDERMEAD", initial_step=0.1, context=ctx, verbose=False)
    assert len(ctx.nlopt) == 1 and ctx.objective == 0


def test_initial_step_errors(monkeypatch, inputs):
    monkeypatch.delenv("KPDI_REFINE_NLOPT", raising=False)
    text = ("The initial step must be a single number when refining orientations or PCs and a list of two numbers when "
            "refining both")
    for mode, step in (("ori", [0.1, 0.2]), ("pc", [0.1, 0.2, 0.3]), ("ori_pc", 0.1), ("ori_pc", [0.1] * 6)):
        ctx = _Recorder()
        with pytest.raises(ValueError) as err:
            rf.refine(mode, *inputs, method="LN_NELDERMEAD", initial_step=step, context=ctx, verbose=False)
        assert str(err.value) == text and ctx.nlopt == []


def test_search_statuses_raise_as_nlopts_binding_does(monkeypatch, inputs):
    monkeypatch.delenv("KPDI_REFINE_NLOPT", raising=False)
    with pytest.raises(RuntimeError, match="failure"):
        rf.refine("ori", *inputs, method="LN_NELDERMEAD", initial_step=0.0, context=_Recorder(status=-1), verbose=False)
    with pytest.raises(ValueError, match="invalid argument"):
        rf.refine("ori", *inputs, method="LN_NELDERMEAD", context=_Recorder(status=-2), verbose=False)
    for ok in (1, 3, 4, 5):
        rf.refine("ori", *inputs, method="LN_NELDERMEAD", context=_Recorder(status=ok), verbose=False)


def test_information_message(monkeypatch, inputs, capsys):
    monkeypatch.delenv("KPDI_REFINE_NLOPT", raising=False)
    rf.refine("ori_pc", *inputs, method="LN_NELDERMEAD", initial_step=[0.1, 0.05], rtol=1e-3, maxeval=200,
              trust_region=[5, 5, 5, 0.05, 0.05, 0.05], context=_Recorder(), compute=False)
    said = capsys.readouterr().out
    assert said == ("Refinement information:\n"
                    "  Method: LN_NELDERMEAD (local) from NLopt, restated on the GPU\n"
                    "  Trust region (+/-): [5.   5.   5.   0.05 0.05 0.05]\n"
                    "  Relative tolerance: 0.001\n"
                    "  Initial step(s): [0.1, 0.1, 0.1, 0.05, 0.05, 0.05]\n"
                    "  Max. function evaulations: 200\n")
    rf.refine("ori", *inputs, method="LN_NELDERMEAD", pseudo_symmetry_ops=np.array([[0.0, 0, 0, 1]]),
              context=_Recorder(), compute=False)
    said = capsys.readouterr().out
    assert said == ("Refinement information:\n"
                    "  Method: LN_NELDERMEAD (local) from NLopt, restated on the GPU\n"
                    "  Trust region (+/-): None\n"
                    "  Relative tolerance: 0.0001\n"
                    "  No. pseudo-symmetry operators: 1\n")


def test_the_pinned_host_plan_is_untouched():
    """`_optimization_plan` still hands ln_neldermead to the host optimiser (ImportError without nlopt)."""
    try:
        import nlopt  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError):
            rf._optimization_plan("ln_neldermead", None, 0.1, 1e-4, None, "ori")
