"""SciPy's differential evolution without a GPU: csrc/differential_evolution.h compiled with the host compiler.  Its
random stream against `numpy.random.RandomState` word for word; the solver over tests/_de_cases.py against
`scipy.optimize.differential_evolution` bit for bit, with every branch of the header reached and four deliberately
wrong variants each failing the table; which `method_kwargs` take the device solver (`_device_de_options`); and the
dispatch of `refine` with a stand-in context."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import _de_cases as dc
from kikuchipy_amd.indexing import _refinement as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The objectives are csrc/analytic_objectives.h (kinds numbered as in tests/_de_cases.py: `analytic_kind_de`), in the
# operation order of tests/_de_cases.py.  Lines on stdin (floats as C99 hex or "nan"):
#   case kind n members maxiter tol atol mutation_lo mutation_hi recombination init updating seed lower[n] upper[n]
#     -> success nfev nit redraws fun x[n]                (floats as their 64 bits)
#   state seed                            -> pos key[624]
#   draws seed rows words (op a b)[rows]  -> the words
# then "count <name> <hits>" per branch.
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "analytic_objectives.h"
#include "differential_evolution.h"

using Analytic = kpdi::AnalyticObjective;

constexpr int CAP = 256;
using Solver = kpdi::DifferentialEvolution<6, CAP, Analytic>;
static Solver::Storage storage;

int main() {
  static char line[1 << 16];
  while (std::fgets(line, sizeof line, stdin)) {
    char *p = line;
    if (!std::strncmp(p, "case ", 5)) {
      p += 5;
      Analytic f;
      f.kind = kpdi::analytic_kind_de((int)std::strtol(p, &p, 10));
      f.n = (int)std::strtol(p, &p, 10);
      const int members = (int)std::strtol(p, &p, 10), maxiter = (int)std::strtol(p, &p, 10);
      const double tol = std::strtod(p, &p), atol = std::strtod(p, &p);
      const double mlo = std::strtod(p, &p), mhi = std::strtod(p, &p), cr = std::strtod(p, &p);
      const int init = (int)std::strtol(p, &p, 10), updating = (int)std::strtol(p, &p, 10);
      const unsigned long seed = std::strtoul(p, &p, 10);
      double lo[6], hi[6];
      if (f.n < 1 || f.n > 6 || members < 5 || members > CAP) return 2;
      for (int i = 0; i < f.n; ++i) lo[i] = std::strtod(p, &p);
      for (int i = 0; i < f.n; ++i) hi[i] = std::strtod(p, &p);
      Solver de(f, storage);
      de.solve(f.n, lo, hi, members, maxiter, tol, atol, mlo, mhi, cr, init, updating, (uint32_t)seed);
      std::printf("%d %lld %d %lld %016llx", (int)de.success, de.nfev, de.nit, de.redraws,
                  (unsigned long long)kpdi::de_bits(de.fun));
      for (int i = 0; i < f.n; ++i) std::printf(" %016llx", (unsigned long long)kpdi::de_bits(de.x[i]));
      std::printf("\n");
    } else if (!std::strncmp(p, "state ", 6)) {
      p += 6;
      kpdi::Mt19937 mt;
      kpdi::mt_seed(mt, (uint32_t)std::strtoul(p, &p, 10));
      std::printf("%d", mt.pos);
      for (int i = 0; i < 624; ++i) std::printf(" %u", mt.key[i]);
      std::printf("\n");
    } else if (!std::strncmp(p, "draws ", 6)) {
      p += 6;
      const unsigned long seed = std::strtoul(p, &p, 10);
      const int rows = (int)std::strtol(p, &p, 10);
      const long long words = std::strtoll(p, &p, 10);
      std::vector<double> program(3 * (size_t)rows);
      for (double &v : program) v = std::strtod(p, &p);
      std::vector<uint64_t> out((size_t)words + 1, 0);
      static int index[CAP], scratch[CAP];
      kpdi::Mt19937 mt;
      kpdi::mt_seed(mt, (uint32_t)seed);
      const long long wrote = kpdi::mt_program(mt, program.data(), rows, index, scratch, CAP, out.data(), words);
      std::printf("%lld", wrote);
      for (long long i = 0; i < words; ++i) std::printf(" %llx", (unsigned long long)out[i]);
      std::printf("\n");
    }
  }
  for (int b = 0; b < kpdi::DEB_COUNT; ++b)
    std::printf("count %s %lld\n", kpdi::kpdi_de_branch_names[b], kpdi::kpdi_de_count[b]);
  return 0;
}
"""

# Branches of differential_evolution.h that no case reaches, with the reason (at most three may be listed).
UNREACHED = {}

SEEDS = (0, 1, 2**32 - 1, 20241020)

# KPDI_DE_WRONG: the deliberately wrong variants of the header, each of which must fail the table
WRONG = {1: "the draw order of _mutate in _mutate_many", 2: "plain instead of pairwise summation",
         3: "< for <= in acceptance (SciPy accepts a trial of equal energy)", 4: "a fresh index array per _select_samples"}


def hexf(v):
    v = float(v)
    return "nan" if v != v else v.hex()


def case_line(i):
    kind, (lower, upper), kw, _ = dc.CASES[i]
    mlo, mhi = dc.mutation_pair(kw.get("mutation", (0.5, 1)))
    words = ["case", kind, len(lower), dc.members(dc.CASES[i]), dc.want(i)[1], hexf(kw.get("tol", 0.01)),
             hexf(kw.get("atol", 0)), hexf(mlo), hexf(mhi), hexf(kw.get("recombination", 0.7)),
             int(kw.get("init", "latinhypercube") == "random"), int(kw.get("updating", "immediate") == "deferred"),
             kw["seed"]]
    words += [hexf(v) for v in lower] + [hexf(v) for v in upper]
    return " ".join(str(w) for w in words)


def program_line(seed, rows):
    return " ".join(["draws", str(seed), str(len(rows)), str(dc.program_words(rows))] +
                    [hexf(v) for v in dc.program_array(rows).ravel()])


def build(tmp, wrong=0):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp / "de_driver.cpp", tmp / f"de_driver_{wrong}"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-DKPDI_DE_COUNT", f"-DKPDI_DE_WRONG={wrong}", "-I",
                    os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return exe


def run(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True)
    out = out.stdout.strip().split("\n")
    rows = [ln.split() for ln in out if not ln.startswith("count ")]
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in out if ln.startswith("count ")}
    assert len(rows) == len(lines)
    return rows, counts


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return tmp_path_factory.mktemp("de")


@pytest.fixture(scope="module")
def driver_output(driver):
    lines = ([f"state {seed}" for seed in SEEDS] + [program_line(*prog) for prog in dc.PROGRAMS] +
             [case_line(i) for i in range(len(dc.CASES))])
    rows, counts = run(build(driver), lines)
    return dict(state=rows[:len(SEEDS)], draws=rows[len(SEEDS):len(SEEDS) + len(dc.PROGRAMS)],
                cases=rows[len(SEEDS) + len(dc.PROGRAMS):], counts=counts)


def from_bits(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------ the random stream
@pytest.mark.parametrize("k", range(len(SEEDS)))
def test_seeding_is_random_states(driver_output, k):
    name, key, pos = np.random.RandomState(SEEDS[k]).get_state()[:3]
    row = driver_output["state"][k]
    assert name == "MT19937" and int(row[0]) == pos == 624
    assert np.array_equal(np.array([int(w) for w in row[1:]], dtype=np.uint32), key)


def test_the_programs_cover_what_the_issue_asks():
    assert any(sum(2 for op, _, _ in rows if op == 0) > 624 for _, rows in dc.PROGRAMS)   # the twist runs
    assert {int(a) for _, rows in dc.PROGRAMS for op, a, _ in rows if op == 2} == {1, 2, 3, 4, 5, 6}
    for op in (3, 4):
        assert {5, 8, 9, 45, 90, 128, 129, dc.DE_POP_MAX} <= {int(a) for _, rows in dc.PROGRAMS for o, a, _ in rows if o == op}
    assert {seed for seed, _ in dc.PROGRAMS} >= {0, 2**32 - 1}


@pytest.mark.parametrize("k", range(len(dc.PROGRAMS)))
def test_draws_are_random_states(driver_output, k):
    seed, rows = dc.PROGRAMS[k]
    want = dc.program_want(seed, rows)
    row = driver_output["draws"][k]
    assert int(row[0]) == want.size == dc.program_words(rows)
    got = np.array([int(w, 16) for w in row[1:]], dtype=np.uint64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:5]


# ------------------------------------------------------------------ the solver
def check_case(row, i):
    """The driver's row of case i against SciPy; returns what differs."""
    want, _ = dc.want(i)
    success, nfev, nit = int(row[0]), int(row[1]), int(row[2])
    fun, x = from_bits(row[4:5])[0], from_bits(row[5:])
    wrong = []
    if (success, nfev, nit) != (int(want.success), want.nfev, want.nit):
        wrong.append(("success, nfev, nit", (success, nfev, nit), (want.success, want.nfev, want.nit)))
    if not dc.same_bits(x, want.x):
        wrong.append(("x", x, want.x))
    if not dc.same_bits(fun, want.fun):
        wrong.append(("fun", fun, want.fun))
    return wrong


@pytest.mark.parametrize("case", range(len(dc.CASES)))
def test_header_matches_scipy_bit_for_bit(driver_output, case):
    row = driver_output["cases"][case]
    (want, maxiter), pinned = dc.want(case), dc.CASES[case][3]
    # the premises of the table: what SciPy 1.15.3 returned when it was written
    assert dc.members(dc.CASES[case]) == pinned["members"] == len(want.population)
    for name in ("nit", "nfev", "success"):
        if name in pinned:
            assert getattr(want, name) == pinned[name], (name, want)
    if pinned.get("last"):
        assert want.nit == maxiter and want.success, "converges in the last generation allowed"
    if pinned.get("redraws"):
        assert int(row[3]) > 0, "no value was drawn again by _ensure_constraint"
    assert not check_case(row, case)


def test_the_table_covers_what_the_issue_asks():
    cases = dc.CASES
    assert {len(c[1][0]) for c in cases} == {1, 2, 3, 4, 5, 6}
    assert {dc.members(c) for c in cases} >= {5, 7, 8, 9, 45, 90, 129, dc.DE_POP_MAX}
    modes = {(c[2].get("updating", "immediate"), c[2].get("init", "latinhypercube")) for c in cases}
    assert len(modes) == 4
    assert {np.ndim(c[2].get("mutation", (0.5, 1))) for c in cases} == {0, 1}
    assert {float(c[2].get("recombination", 0.7)) for c in cases} >= {0.0, 0.7, 1.0}
    assert any(c[2].get("tol") == 0 and c[2].get("atol") == 0 and c[3].get("success") is False for c in cases)
    assert any(c[0] == 7 and c[3].get("nit") == 1 for c in cases) and any(c[3].get("last") for c in cases)
    assert any(c[3].get("redraws") for c in cases)
    assert any(np.any(np.equal(*c[1])) for c in cases)
    assert {3, 4} <= {c[0] for c in cases}
    for u in ("immediate", "deferred"):
        assert any(c[0] == 4 and c[2]["maxiter"] <= 3 and c[2].get("updating", "immediate") == u for c in cases)
    # the objectives in Python are the driver's: same values at a point off every special case
    x = np.array([0.37, 1.21, 0.55, 1.93, 0.08, 1.4])
    assert dc.OBJECTIVES[5](x) == dc.hug(x) > 0 and dc.OBJECTIVES[7](x) == 0.1 and np.isinf(dc.OBJECTIVES[6](x))


def test_every_branch_of_the_header_is_reached(driver_output):
    counts = driver_output["counts"]
    assert len(UNREACHED) <= 3 and set(UNREACHED) <= set(counts)
    missed = sorted(name for name, hits in counts.items() if hits == 0 and name not in UNREACHED)
    assert not missed, missed
    assert all(counts[name] == 0 for name in UNREACHED), "a branch listed as unreachable was reached: take it off the list"


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_a_wrong_variant_fails_the_table(driver, driver_output, wrong):
    rows, _ = run(build(driver, wrong), [case_line(i) for i in range(len(dc.CASES))])
    failed = [i for i in range(len(dc.CASES)) if check_case(rows[i], i)]
    assert failed, WRONG[wrong]
    print(WRONG[wrong], "fails cases", failed)


# ------------------------------------------------------------------ which calls take the device solver
def _host(_optimiser="differential_evolution", **method_kwargs):
    return rf._optimization_plan(_optimiser, method_kwargs or None, None, 1e-4, None, "ori")[1]


DEFAULTS = dict(maxiter=1000, popsize=15, tol=0.01, atol=0.0, mutation=(0.5, 1.0), recombination=0.7, seed=None,
                polish=True, init=0, updating=0)


def test_device_de_options_taken():
    assert rf._device_de_options(_host()) == DEFAULTS
    for kwargs, changed in [
        (dict(strategy="best1bin"), {}),
        (dict(maxiter=12), dict(maxiter=12)),
        (dict(maxiter=0), dict(maxiter=0)),
        (dict(maxiter=None), {}),                      # "the default used to be None"
        (dict(popsize=8), dict(popsize=8)),
        (dict(tol=1e-6), dict(tol=1e-6)),
        (dict(atol=1e-3), dict(atol=1e-3)),
        (dict(mutation=0.8), dict(mutation=(0.8, float("nan")))),
        (dict(mutation=(1.0, 0.4)), dict(mutation=(0.4, 1.0))),   # SciPy sorts the pair
        (dict(mutation=[0.5, 0.5]), dict(mutation=(0.5, 0.5))),
        (dict(recombination=0), dict(recombination=0.0)),
        (dict(recombination=1), dict(recombination=1.0)),
        (dict(seed=None), {}),
        (dict(seed=0), dict(seed=0)),
        (dict(seed=np.int64(2**32 - 1)), dict(seed=2**32 - 1)),
        (dict(polish=False), dict(polish=False)),
        (dict(init="latinhypercube"), {}),
        (dict(init="random"), dict(init=1)),
        (dict(updating="immediate"), {}),
        (dict(updating="deferred"), dict(updating=1)),
        (dict(disp=False), {}),
    ]:
        got = rf._device_de_options(_host(**kwargs))
        want = dict(DEFAULTS, **changed)
        assert got is not None, kwargs
        assert repr(got) == repr(want), (kwargs, got)   # repr: NaN compares unequal


def test_device_de_options_declined():
    for kwargs in (dict(rng=1), dict(seed=np.random.RandomState(1)), dict(seed=np.random.default_rng(1)),
                   dict(callback=print), dict(workers=2), dict(workers=1), dict(constraints=()), dict(x0=[0, 0, 0]),
                   dict(integrality=[True, False, False]), dict(vectorized=True), dict(vectorized=False),
                   dict(strategy="rand1bin"), dict(strategy="best1exp"), dict(strategy=lambda c, p, rng=None: p[c]),
                   dict(init="sobol"), dict(init="halton"), dict(init=np.zeros((5, 3))), dict(init="nonsense"),
                   dict(updating="sometimes"), dict(disp=True), dict(args=()), dict(maxfun=100), dict(unknown=1),
                   # invalid values stay with SciPy, which raises its own errors
                   dict(mutation=2.0), dict(mutation=-0.1), dict(mutation=(0.5, 2.0)), dict(mutation=float("nan")),
                   dict(mutation=(0.5,)), dict(mutation=(0.1, 0.2, 0.3)), dict(mutation="0.5"),
                   dict(seed=-1), dict(seed=2**32), dict(seed=1.5), dict(seed=True),
                   dict(maxiter=-1), dict(maxiter=2.5), dict(maxiter=2**31), dict(maxiter=float("inf")),
                   dict(popsize=0), dict(popsize=2.5), dict(popsize=-3),
                   dict(tol=float("nan")), dict(tol="x"), dict(atol=float("inf")), dict(atol=None),
                   dict(recombination=float("nan")), dict(recombination=None),
                   dict(polish=1), dict(polish=None)):
        assert rf._device_de_options(_host(**kwargs)) is None, kwargs
    assert rf._device_de_options(_host("dual_annealing", seed=3)) is None
    assert rf._device_de_options(_host("minimize", method="Powell")) is None
    assert rf._device_de_options(None) is None
    # the plan itself is what it was: a host optimiser and the reference's message
    nm, host, plan = rf._optimization_plan("differential_evolution", dict(seed=1), None, 1e-4, None, "ori")
    assert nm is None and isinstance(host, rf._HostOptimizer) and plan["method_name"] == "differential_evolution"
    info = rf._info_message("ori", [1, 1, 1], plan["kwargs"], 0, plan)
    assert info == ("Refinement information:\n  Method: differential_evolution (global) from SciPy\n"
                    "  Trust region (+/-): [1 1 1]\n  Keyword arguments passed to method: {'seed': 1}")


def test_population_and_seeds():
    lower, upper = np.zeros((2, 3, 3)), np.ones((2, 3, 3))
    assert rf._de_members(15, lower, upper) == 45 and rf._de_members(1, lower, upper) == 5
    upper[:, :, 1] = 0
    assert rf._de_members(15, lower, upper) == 30
    upper[0, 0, 2] = 0
    assert rf._de_members(15, lower, upper) is None   # the jobs differ: the host works each out
    assert rf._de_members(15, np.zeros((1, 1, 6)), np.ones((1, 1, 6))) == 90
    assert rf._de_members(43, np.zeros((1, 1, 6)), np.ones((1, 1, 6))) is None   # 258 members: above the cap
    assert rf._de_members(64, np.zeros((1, 1, 4)), np.ones((1, 1, 4))) == rf.DE_POP_MAX == dc.DE_POP_MAX
    seeds = rf._de_seeds(7, 6)
    assert seeds.dtype == np.uint32 and np.array_equal(seeds, [7] * 6)
    fresh, again = rf._de_seeds(None, 6), rf._de_seeds(None, 6)
    assert fresh.dtype == np.uint32 and fresh.shape == (6,) and len(set(fresh)) == 6 and not np.array_equal(fresh, again)


class _Recorder:
    """Stands in for the engine context of `refine`: records the solver and objective calls."""

    def __init__(self):
        self.de, self.objective = [], 0

    def set_master_pattern(self, up, lo):
        pass

    def refine_set_patterns(self, pats, signal_mask, rescale, om):
        pass

    def refine_solve_de(self, mode, fixed, lower, upper, members, maxiter, tol, atol, mutation, recombination, init,
                        updating, seeds):
        self.de.append(dict(mode=mode, shape=lower.shape, members=members, maxiter=maxiter, tol=tol, atol=atol,
                            mutation=mutation, recombination=recombination, init=init, updating=updating,
                            seeds=np.array(seeds)))
        out = np.zeros(lower.shape[:2] + (3 + lower.shape[2],))
        out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3:] = 0.75, 77, 3, 0.5 * (lower + upper)
        return out

    def refine_objective(self, mode, pattern_index, x, fixed=None):
        self.objective += len(pattern_index)
        return np.array([0.5 + float(np.sum((np.asarray(xx) - 0.1) ** 2)) for xx in x])


def test_refine_sends_plain_differential_evolution_to_the_device(monkeypatch):
    import kikuchipy_amd as ka

    det = ka.EBSDDetector(shape=(6, 6), pc=(0.4, 0.6, 0.5))
    mp = ka.EBSDMasterPattern(np.random.default_rng(0).random((11, 11), dtype=np.float32))
    pats = np.random.default_rng(1).integers(0, 255, (2, 3, 6, 6), dtype=np.uint8)
    rot = np.tile([1.0, 0, 0, 0], (2, 3, 1))
    monkeypatch.delenv("KPDI_REFINE_DE", raising=False)

    def run(mode="ori", contexts=None, trust_region=(1, 1, 1), **method_kwargs):
        ctx = _Recorder()
        kw = dict(contexts=contexts(ctx)) if contexts else dict(context=ctx)
        res = rf.refine(mode, pats, rot, det, mp, method="differential_evolution", method_kwargs=method_kwargs,
                        verbose=False, trust_region=list(trust_region), **kw)
        return ctx, res

    ctx, (res, _) = run(seed=5, polish=False, popsize=4, maxiter=9, tol=1e-3, mutation=0.7, updating="deferred")
    assert ctx.objective == 0 and len(ctx.de) == 1, "polish=False makes no objective call from the host"
    call = ctx.de[0]
    assert (call["mode"], call["shape"], call["members"], call["maxiter"]) == (rf.MODES["ori"], (6, 1, 3), 12, 9)
    assert (call["tol"], call["atol"], call["recombination"], call["init"], call["updating"]) == (1e-3, 0.0, 0.7, 0, 1)
    assert call["mutation"][0] == 0.7 and np.isnan(call["mutation"][1])
    assert call["seeds"].dtype == np.uint32 and np.array_equal(call["seeds"], [5] * 6)   # every job starts from RandomState(5)
    assert np.array_equal(res.num_evals, [77] * 6) and np.allclose(res.scores, 0.25)
    # seed=None: one fresh seed per job
    ctx, _ = run(polish=False, maxiter=2)
    assert ctx.objective == 0 and ctx.de[0]["seeds"].shape == (6,) and len(set(ctx.de[0]["seeds"])) == 6
    # the default polish: the evolution on the device, then L-BFGS-B on the host with the objective through the context
    ctx, (res, _) = run(seed=5, maxiter=2)
    assert len(ctx.de) == 1 and ctx.objective > 0
    assert np.all(res.num_evals > 77) and np.all(res.scores > 0.25)   # nfev += result.nfev; the better point is taken
    # the combined refinement has six variables; one call per block of points
    ctx, _ = run("ori_pc", trust_region=(1, 1, 1, 0.01, 0.01, 0.01), seed=5, polish=False)
    assert ctx.de[0]["shape"] == (6, 1, 6) and ctx.de[0]["members"] == 90
    ctx, _ = run(contexts=lambda c: [c, c], seed=5, polish=False)
    assert [call["shape"] for call in ctx.de] == [(3, 1, 3), (3, 1, 3)] and ctx.objective == 0
    assert [list(call["seeds"]) for call in ctx.de] == [[5] * 3, [5] * 3]
    # what the device solver does not restate: SciPy on the host, the objective through the context
    for kwargs in (dict(strategy="rand1bin"), dict(popsize=90), dict(init="sobol")):
        ctx, _ = run(seed=5, polish=False, maxiter=1, **kwargs)
        assert ctx.de == [] and ctx.objective > 0, kwargs
    monkeypatch.setenv("KPDI_REFINE_DE", "host")
    ctx, _ = run(seed=5, polish=False, maxiter=1, popsize=2)
    assert ctx.de == [] and ctx.objective == 6 * 2 * 6   # six jobs, the population of 6 and one generation
    monkeypatch.setenv("KPDI_REFINE_DE", "device")   # anything but "host"
    ctx, _ = run(seed=5, polish=False, maxiter=1, popsize=2)
    assert len(ctx.de) == 1 and ctx.objective == 0
