"""SciPy's basinhopping without a GPU: csrc/basinhopping.h compiled with the host compiler, over
tests/_basinhopping_cases.py against `scipy.optimize.basinhopping` bit for bit, with every branch of the header
reached; the condition on the table's inputs that keeps the Metropolis test away from the rounding of `exp`; which
`method_kwargs` take the device solver (`_device_basinhopping_options`); and the dispatch of `refine` with a stand-in
context."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import _basinhopping_cases as bc
from kikuchipy_amd.indexing import _refinement as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The objectives are csrc/analytic_objectives.h, kinds 0..4.  Lines on stdin (floats as C99 hex or "nan"):
#   case kind n niter T stepsize interval niter_success target_accept_rate stepwise_factor xatol fatol maxiter maxfun
#        seed x0[n]                 (niter_success -1: None; maxiter, maxfun: the resolved budget)
#     -> success nfev nit minimization_failures fun x[n]      (floats as their 64 bits)
# then "count <name> <hits>" per branch.
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "analytic_objectives.h"
#include "basinhopping.h"

int main() {
  static char line[1 << 12];
  static kpdi::Mt19937 mt;
  static kpdi::BasinHopping<6> bh;
  while (std::fgets(line, sizeof line, stdin)) {
    char *p = line;
    if (std::strncmp(p, "case ", 5)) continue;
    p += 5;
    kpdi::AnalyticObjective f;
    f.kind = (int)std::strtol(p, &p, 10);
    f.n = (int)std::strtol(p, &p, 10);
    const int niter = (int)std::strtol(p, &p, 10);
    const double T = std::strtod(p, &p), stepsize = std::strtod(p, &p);
    const int interval = (int)std::strtol(p, &p, 10);
    const long long niter_success = std::strtoll(p, &p, 10);
    const double target = std::strtod(p, &p), factor = std::strtod(p, &p);
    const double xatol = std::strtod(p, &p), fatol = std::strtod(p, &p);
    const int maxiter = (int)std::strtol(p, &p, 10), maxfun = (int)std::strtol(p, &p, 10);
    const unsigned long seed = std::strtoul(p, &p, 10);
    double x0[6];
    if (f.n < 1 || f.n > 6 || interval < 1 || niter < 0 || maxiter < 1 || maxfun < 1) return 2;
    for (int i = 0; i < f.n; ++i) x0[i] = std::strtod(p, &p);
    kpdi::mt_seed(mt, (uint32_t)seed);
    bh.begin(mt, f.n, x0, niter, T, stepsize, interval, niter_success, target, factor, xatol, fatol, maxiter, maxfun);
    while (bh.state != kpdi::BasinHopping<6>::S_DONE) bh.feed(mt, f.eval(bh.xeval()));
    std::printf("%d %lld %d %d %016llx", (int)bh.success, bh.nfev, bh.nit, bh.minimization_failures,
                (unsigned long long)kpdi::de_bits(bh.fun));
    for (int i = 0; i < f.n; ++i) std::printf(" %016llx", (unsigned long long)kpdi::de_bits(bh.xbest[i]));
    std::printf("\n");
  }
  for (int b = 0; b < kpdi::BHB_COUNT; ++b)
    std::printf("count %s %lld\n", kpdi::kpdi_bh_branch_names[b], kpdi::kpdi_bh_count[b]);
  return 0;
}
"""


def hexf(v):
    v = float(v)
    return "nan" if v != v else v.hex()


def case_line(i):
    kind, x0, kw, _ = bc.CASES[i]
    xatol, fatol, maxiter, maxfev = bc.quench_options(bc.CASES[i])
    it, fev = bc.budget(len(x0), maxiter, maxfev)
    ns = kw.get("niter_success")
    words = ["case", kind, len(x0), kw.get("niter", 100), hexf(kw.get("T", 1.0)), hexf(kw.get("stepsize", 0.5)),
             kw.get("interval", 50), -1 if ns is None else ns, hexf(kw.get("target_accept_rate", 0.5)),
             hexf(kw.get("stepwise_factor", 0.9)), hexf(xatol), hexf(fatol), it, fev, kw["seed"]]
    words += [hexf(v) for v in x0]
    return " ".join(str(w) for w in words)


def build(tmp):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp / "bh_driver.cpp", tmp / "bh_driver"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-DKPDI_BH_COUNT", "-I",
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
def driver_output(tmp_path_factory):
    rows, counts = run(build(tmp_path_factory.mktemp("bh")), [case_line(i) for i in range(len(bc.CASES))])
    return dict(cases=rows, counts=counts)


def from_bits(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


# ------------------------------------------------------------------ the header against SciPy
@pytest.mark.parametrize("case", range(len(bc.CASES)))
def test_header_matches_scipy_bit_for_bit(driver_output, case):
    row = driver_output["cases"][case]
    (want, hops), pinned = bc.want(case), bc.CASES[case][3]
    niter = bc.CASES[case][2]["niter"]
    # the premises of the table: what SciPy 1.15.3 returned when it was written
    assert len(hops) == (want.nit if niter else 0)
    for name, attr in (("nit", "nit"), ("nfev", "nfev"), ("success", "success"), ("failures", "minimization_failures")):
        if name in pinned:
            assert getattr(want, attr) == pinned[name], (name, want)
    if pinned.get("early"):
        assert want.nit < niter and want.message == ["success condition satisfied"]
    if pinned.get("mixed"):
        assert 0 < want.minimization_failures < want.nit + 1, "some quenches fail, some succeed"
    if pinned.get("both_ways"):
        sizes = bc.step_sizes(bc.CASES[case])
        assert min(sizes) < bc.CASES[case][2].get("stepsize", 0.5) < max(sizes), sizes
    success, nfev, nit, failures = (int(w) for w in row[:4])
    fun, x = from_bits(row[4:5])[0], from_bits(row[5:])
    assert (success, nfev, nit, failures) == (int(want.success), want.nfev, want.nit, want.minimization_failures), (row, want)
    assert bc.same_bits(x, want.x), (x, want.x)
    assert bc.same_bits(fun, want.fun), (fun, want.fun)


@pytest.mark.parametrize("case", range(len(bc.CASES)))
def test_metropolis_is_never_decided_by_the_rounding_of_exp(case):
    _, hops = bc.want(case)
    assert bc.margin_ok(hops), [(w, draw) for w, draw in hops if 0 < w < 1 and abs(w - draw) <= bc.MARGIN]


def test_the_table_covers_what_the_issue_asks():
    cases = bc.CASES
    assert {len(c[1]) for c in cases} >= {1, 3, 6}
    assert any(c[2].get("T") == 0 for c in cases)
    assert any(c[2].get("interval") == 2 and c[3].get("both_ways") for c in cases)
    assert any(c[2].get("niter_success") is not None and c[3].get("early") for c in cases)
    assert any(c[3].get("success") is False and c[3].get("failures") for c in cases) and any(c[3].get("mixed") for c in cases)
    assert any(c[2]["niter"] == 0 for c in cases)
    assert any(c[0] == 4 for c in cases)
    assert {0, 2**32 - 1} <= {c[2]["seed"] for c in cases}
    assert any(0 < w < 1 for i in range(len(cases)) for w, _ in bc.want(i)[1]), "no hop is decided by exp at all"
    gpu = [cases[i] for i in bc.GPU_CASES]
    assert {1, 6} <= {len(c[1]) for c in gpu}


def test_every_branch_of_the_header_is_reached(driver_output):
    counts = driver_output["counts"]
    assert len(counts) == 30
    missed = sorted(name for name, hits in counts.items() if hits == 0)
    assert not missed, missed


# ------------------------------------------------------------------ which calls take the device solver
NM = dict(method="Nelder-Mead")


def _host(_optimiser="basinhopping", **method_kwargs):
    return rf._optimization_plan(_optimiser, method_kwargs or None, None, 1e-4, None, "ori")[1]


DEFAULTS = dict(niter=100, T=1.0, stepsize=0.5, interval=50, niter_success=None, seed=None, target_accept_rate=0.5,
                stepwise_factor=0.9, xatol=1e-4, fatol=1e-4, maxiter=None, maxfev=None)


def test_device_basinhopping_options_taken():
    assert rf._device_basinhopping_options(_host(minimizer_kwargs=NM)) == DEFAULTS
    for kwargs, changed in [
        (dict(niter=0), dict(niter=0)),
        (dict(niter=np.int64(7)), dict(niter=7)),
        (dict(T=0), dict(T=0.0)),
        (dict(T=2.5), dict(T=2.5)),
        (dict(T=-1.0), dict(T=-1.0)),
        (dict(stepsize=0.01), dict(stepsize=0.01)),
        (dict(interval=1), dict(interval=1)),
        (dict(interval=2), dict(interval=2)),
        (dict(niter_success=None), {}),
        (dict(niter_success=0), dict(niter_success=0)),
        (dict(niter_success=3), dict(niter_success=3)),
        (dict(seed=None), {}),
        (dict(seed=0), dict(seed=0)),
        (dict(seed=np.int64(2**32 - 1)), dict(seed=2**32 - 1)),
        (dict(target_accept_rate=0.9), dict(target_accept_rate=0.9)),
        (dict(stepwise_factor=0.5), dict(stepwise_factor=0.5)),
        (dict(disp=False), {}),
    ]:
        got = rf._device_basinhopping_options(_host(minimizer_kwargs=NM, **kwargs))
        assert got == dict(DEFAULTS, **changed), (kwargs, got)
    for mk, changed in [
        (dict(method="nelder-mead"), {}),
        (dict(method="Nelder-Mead", tol=1e-6), dict(xatol=1e-6, fatol=1e-6)),
        (dict(method="Nelder-Mead", tol=1e-6, options=dict(xatol=1e-3)), dict(xatol=1e-3, fatol=1e-6)),
        (dict(method="Nelder-Mead", options=dict(fatol=1e-2, maxiter=30)), dict(fatol=1e-2, maxiter=30)),
        (dict(method="Nelder-Mead", options=dict(maxfev=60, disp=False)), dict(maxfev=60)),
        (dict(method="Nelder-Mead", options=dict(maxiter=None, maxfev=None)), {}),
        (dict(method="Nelder-Mead", options=None), {}),
    ]:
        got = rf._device_basinhopping_options(_host(minimizer_kwargs=mk))
        assert got == dict(DEFAULTS, **changed), (mk, got)


def test_device_basinhopping_options_declined():
    for kwargs in (dict(take_step=lambda x: x), dict(accept_test=lambda **kw: True), dict(callback=print), dict(rng=1),
                   dict(seed=np.random.RandomState(1)), dict(seed=np.random.default_rng(1)), dict(disp=True),
                   dict(unknown=1), dict(x0=[0, 0, 0]),
                   # invalid or unusual values stay with SciPy, which runs or raises as it does today
                   dict(interval=0), dict(interval=-1), dict(interval=2.0), dict(interval=True), dict(interval=None),
                   dict(niter=-1), dict(niter=2.5), dict(niter=2**31), dict(niter=None), dict(niter=True),
                   dict(niter_success=-1), dict(niter_success=1.5),
                   dict(T=float("nan")), dict(T=float("inf")), dict(T="1"), dict(T=None),
                   dict(stepsize=float("nan")), dict(stepsize=float("inf")), dict(stepsize=None), dict(stepsize=1e308),
                   dict(target_accept_rate=0.0), dict(target_accept_rate=1.0), dict(target_accept_rate=float("nan")),
                   dict(stepwise_factor=0.0), dict(stepwise_factor=1.0), dict(stepwise_factor=1.5),
                   dict(seed=-1), dict(seed=2**32), dict(seed=1.5), dict(seed=True)):
        assert rf._device_basinhopping_options(_host(minimizer_kwargs=NM, **kwargs)) is None, kwargs
    for mk in (None, {}, dict(tol=1e-3), dict(method="BFGS"), dict(method="Powell"), dict(method="neldermead"),
               dict(method=lambda fun, x0, **kw: None), dict(method="Nelder-Mead", bounds=[(0, 1)] * 3),
               dict(method="Nelder-Mead", callback=print), dict(method="Nelder-Mead", args=()),
               dict(method="Nelder-Mead", jac=None), dict(method="Nelder-Mead", options=dict(adaptive=True)),
               dict(method="Nelder-Mead", options=dict(return_all=False)),
               dict(method="Nelder-Mead", options=dict(initial_simplex=np.zeros((4, 3)))),
               dict(method="Nelder-Mead", options=dict(bounds=None)), dict(method="Nelder-Mead", options=dict(disp=True)),
               dict(method="Nelder-Mead", options=dict(maxiter=0)), dict(method="Nelder-Mead", options=dict(maxfev=-3)),
               dict(method="Nelder-Mead", options=dict(maxfev=float("inf"))), dict(method="Nelder-Mead", options=dict(maxiter=2.5)),
               dict(method="Nelder-Mead", options=dict(xatol=float("nan"))), dict(method="Nelder-Mead", options=dict(fatol="x")),
               dict(method="Nelder-Mead", tol="x"), dict(method="Nelder-Mead", options=[("maxfev", 3)])):
        kwargs = {} if mk is None else dict(minimizer_kwargs=mk)
        assert rf._device_basinhopping_options(_host(seed=1, **kwargs)) is None, mk
    assert rf._device_basinhopping_options(_host("differential_evolution", seed=3)) is None
    assert rf._device_basinhopping_options(_host("minimize", method="Powell")) is None
    assert rf._device_basinhopping_options(None) is None
    # the plan itself is what it was: a host optimiser and the reference's message
    nm, host, plan = rf._optimization_plan("basinhopping", dict(minimizer_kwargs=NM), None, 1e-4, None, "ori")
    assert nm is None and isinstance(host, rf._HostOptimizer) and plan["method_name"] == "basinhopping"
    info = rf._info_message("ori", None, plan["kwargs"], 0, plan)
    assert info == ("Refinement information:\n  Method: basinhopping (global) from SciPy\n"
                    "  Keyword arguments passed to method: {'minimizer_kwargs': {'method': 'Nelder-Mead'}}")


class _Recorder:
    """Stands in for the engine context of `refine`: records the solver and objective calls."""

    def __init__(self):
        self.bh, self.objective = [], 0

    def set_master_pattern(self, up, lo):
        pass

    def refine_set_patterns(self, pats, signal_mask, rescale, om):
        pass

    def refine_solve_basinhopping(self, mode, x0, fixed, niter, T, stepsize, interval, niter_success, target_accept_rate,
                                  stepwise_factor, xatol, fatol, maxiter, maxfev, seeds):
        self.bh.append(dict(mode=mode, shape=x0.shape, niter=niter, T=T, stepsize=stepsize, interval=interval,
                            niter_success=niter_success, target_accept_rate=target_accept_rate,
                            stepwise_factor=stepwise_factor, xatol=xatol, fatol=fatol, maxiter=maxiter, maxfev=maxfev,
                            seeds=np.array(seeds)))
        out = np.zeros(x0.shape[:2] + (3 + x0.shape[2],))
        out[:, :, 0], out[:, :, 1], out[:, :, 2], out[:, :, 3:] = 0.75, 77, 3, x0
        out[:, 1:, 0], out[:, 1:, 1] = 0.5, 55   # a later start is the better one
        return out

    def refine_objective(self, mode, pattern_index, x, fixed=None):
        self.objective += len(pattern_index)
        return np.array([0.5 + float(np.sum((np.asarray(xx) - 0.1) ** 2)) for xx in x])


def test_refine_sends_plain_basinhopping_to_the_device(monkeypatch):
    import kikuchipy_amd as ka

    det = ka.EBSDDetector(shape=(6, 6), pc=(0.4, 0.6, 0.5))
    mp = ka.EBSDMasterPattern(np.random.default_rng(0).random((11, 11), dtype=np.float32))
    pats = np.random.default_rng(1).integers(0, 255, (2, 3, 6, 6), dtype=np.uint8)
    rot = np.tile([1.0, 0, 0, 0], (2, 3, 1))
    monkeypatch.delenv("KPDI_REFINE_BASINHOPPING", raising=False)

    def run(mode="ori", contexts=None, minimizer_kwargs=NM, **kwargs):
        ctx = _Recorder()
        method_kwargs = {k: kwargs.pop(k) for k in list(kwargs) if k not in ("pseudo_symmetry_ops", "navigation_mask", "comm")}
        if minimizer_kwargs is not None:
            method_kwargs["minimizer_kwargs"] = minimizer_kwargs
        kw = dict(contexts=contexts(ctx)) if contexts else dict(context=ctx)
        res = rf.refine(mode, pats, rot, det, mp, method="basinhopping", method_kwargs=method_kwargs, verbose=False,
                        **kw, **kwargs)
        return ctx, res

    ctx, (res, _) = run(seed=5, niter=4, T=0.5, stepsize=0.01, interval=2, niter_success=3, target_accept_rate=0.4,
                        stepwise_factor=0.8, minimizer_kwargs=dict(method="Nelder-Mead", tol=1e-3, options=dict(maxfev=40)))
    assert ctx.objective == 0 and len(ctx.bh) == 1, "no objective call from the host"
    call = ctx.bh[0]
    assert (call["mode"], call["shape"], call["niter"], call["interval"], call["niter_success"]) == (rf.MODES["ori"], (6, 1, 3), 4, 2, 3)
    assert (call["T"], call["stepsize"], call["target_accept_rate"], call["stepwise_factor"]) == (0.5, 0.01, 0.4, 0.8)
    assert (call["xatol"], call["fatol"], call["maxiter"], call["maxfev"]) == (1e-3, 1e-3, None, 40)
    assert call["seeds"].dtype == np.uint32 and np.array_equal(call["seeds"], [5] * 6)   # every job starts from RandomState(5)
    assert np.array_equal(res.num_evals, [77] * 6) and np.allclose(res.scores, 0.25)
    # seed=None: one fresh seed per job
    ctx, _ = run(niter=2)
    assert ctx.objective == 0 and ctx.bh[0]["seeds"].shape == (6,) and len(set(ctx.bh[0]["seeds"])) == 6
    assert ctx.bh[0]["niter_success"] is None and ctx.bh[0]["maxfev"] is None and ctx.bh[0]["maxiter"] is None
    # pseudo-symmetry starts: one job per (pattern, start); the best start and ITS number of evaluations
    op = np.array([[np.cos(0.1), 0, 0, np.sin(0.1)]])
    ctx, (res, _) = run(seed=5, pseudo_symmetry_ops=op)
    assert ctx.bh[0]["shape"] == (6, 2, 3) and len(ctx.bh[0]["seeds"]) == 12
    assert np.array_equal(res.pseudo_symmetry_index, [1] * 6) and np.array_equal(res.num_evals, [55] * 6)
    # the combined refinement has six variables; the PC refinement three; one call per block of points
    ctx, _ = run("ori_pc", seed=5)
    assert ctx.bh[0]["shape"] == (6, 1, 6) and ctx.bh[0]["mode"] == rf.MODES["ori_pc"]
    ctx, _ = run("pc", seed=5)
    assert ctx.bh[0]["shape"] == (6, 1, 3) and ctx.bh[0]["mode"] == rf.MODES["pc"]
    ctx, _ = run(contexts=lambda c: [c, c], seed=5)
    assert [call["shape"] for call in ctx.bh] == [(3, 1, 3), (3, 1, 3)] and ctx.objective == 0
    assert [list(call["seeds"]) for call in ctx.bh] == [[5] * 3, [5] * 3]
    nav = np.array([[False, True, False], [True, False, False]])
    ctx, (res, _) = run(seed=5, navigation_mask=nav)
    assert ctx.bh[0]["shape"] == (4, 1, 3) and res.scores.shape == (4,)

    class Rank1of2:   # the `comm` route: this rank solves its block, all ranks hold every row
        rank, world_size = 1, 2

        @staticmethod
        def all_gather_rows(rows):
            return np.concatenate([rows, rows], axis=0)

    ctx, (res, _) = run(seed=5, comm=Rank1of2)
    assert [call["shape"] for call in ctx.bh] == [(3, 1, 3)] and ctx.objective == 0 and res.scores.shape == (6,)
    # what the device solver does not restate: SciPy on the host, the objective through the context
    for kwargs in (dict(minimizer_kwargs=dict(method="Powell", options=dict(maxfev=5))), dict(callback=lambda x, f, a: None),
                   dict(minimizer_kwargs=dict(method="Nelder-Mead", options=dict(maxfev=5, adaptive=True)))):
        ctx, _ = run(seed=5, niter=1, **kwargs)
        assert ctx.bh == [] and ctx.objective > 0, kwargs
    monkeypatch.setenv("KPDI_REFINE_BASINHOPPING", "host")
    ctx, _ = run(seed=5, niter=1, minimizer_kwargs=dict(method="Nelder-Mead", options=dict(maxfev=5)))
    assert ctx.bh == [] and ctx.objective == 6 * 2 * 5   # six jobs, two quenches of five evaluations
    monkeypatch.setenv("KPDI_REFINE_BASINHOPPING", "device")   # anything but "host"
    ctx, _ = run(seed=5, niter=1)
    assert len(ctx.bh) == 1 and ctx.objective == 0


def test_deferred_computation_runs_the_device_solver_later(monkeypatch):
    import kikuchipy_amd as ka

    det = ka.EBSDDetector(shape=(6, 6), pc=(0.4, 0.6, 0.5))
    mp = ka.EBSDMasterPattern(np.random.default_rng(0).random((11, 11), dtype=np.float32))
    pats = np.random.default_rng(1).integers(0, 255, (4, 6, 6), dtype=np.uint8)
    monkeypatch.delenv("KPDI_REFINE_BASINHOPPING", raising=False)
    ctx = _Recorder()
    later = rf.refine("ori", pats, np.tile([1.0, 0, 0, 0], (4, 1)), det, mp, method="basinhopping",
                      method_kwargs=dict(seed=1, niter=2, minimizer_kwargs=NM), verbose=False, context=ctx, compute=False)
    assert ctx.bh == []
    res = rf.compute_refine_orientation_results(later)
    assert len(ctx.bh) == 1 and ctx.objective == 0 and res.scores.shape == (4,)
