"""The projection-centre search without a GPU: csrc/hough_search.h - the objective of one pattern and
the resumable Nelder-Mead search around it - and `hough_search_plan` of csrc/hough_plan.h under the host compiler, behind a
small shim loaded with ctypes.  `scipy.optimize.minimize(method="Nelder-Mead")` over the shim's objective and
`hv_pc_search_advance` must return the same `x`, `fun`, `nfev` and `nit` bit for bit, however the search is cut into
launches.  Band sets are made from the synthetic normals of tests/_hough_cases.py, turned into (theta, rho) records under
a known projection centre."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import minimize

import _hough_cases as cases
from kikuchipy_amd import _lib

SHIM = r"""
#include "hough_search.h"
using namespace kpdi;
namespace {
HvPhase phase(int P, int nf, const double *normals, const int32_t *family, const double *angles, double tol) {
  return HvPhase{P, nf, normals, family, angles, tol};
}
HvDetector detector(int ny, int nx, const double *s2d) {
  HvDetector d{};
  d.ny = ny, d.nx = nx;
  for (int k = 0; k < 9; ++k) d.s2d[k] = s2d[k];
  return d;
}
}
extern "C" {
int shim_state_bytes() { return (int)sizeof(HoughPcSearch); }
double shim_objective(const HoughBand *bands, int n_bands, const double *pc, int ny, int nx, const double *s2d, int P, int nf,
                      const double *normals, const int32_t *family, const double *angles, double tol, double tol_deg) {
  return hv_pc_objective(bands, n_bands, pc, detector(ny, nx, s2d), phase(P, nf, normals, family, angles, tol), tol_deg);
}
// the whole search in calls of at most max_evals evaluations each; returns the number of calls, -1 if it never ended
int shim_search(const HoughBand *bands, int n_bands, int ny, int nx, const double *s2d, int P, int nf, const double *normals,
                const int32_t *family, const double *angles, double tol, double tol_deg, const double *pc0, double xatol,
                double fatol, int maxiter, int maxfun, int max_evals, int max_calls, double *x, double *fun, int *counts) {
  HoughPcSearchOptions o{};
  for (int k = 0; k < 3; ++k) o.pc0[k] = pc0[k];
  o.xatol = xatol, o.fatol = fatol, o.maxiter = maxiter, o.maxfun = maxfun, o.tol_deg = tol_deg;
  const HvDetector det = detector(ny, nx, s2d);
  const HvPhase ph = phase(P, nf, normals, family, angles, tol);
  HoughPcSearch s{};  // all zero: not begun
  int calls = 0;
  bool done = false;
  for (; calls < max_calls && !done; ++calls) {
    done = hv_pc_search_advance(s, bands, n_bands, det, ph, o, max_evals);
    if (done != hv_pc_search_done(s)) return -2;
    if (!done && s.nm.fcalls > (calls + 1) * max_evals + 1) return -3;  // (begin asks for the first point)
  }
  if (!done) return -1;
  for (int k = 0; k < 3; ++k) x[k] = s.nm.sim[0][k];
  *fun = s.nm.fun();
  counts[0] = s.nm.fcalls, counts[1] = s.nm.iterations, counts[2] = hv_pc_search_status(s);
  return calls;
}
void shim_plan(int64_t m, int n_cu, int forced, int64_t *out) {
  const HoughSearchPlan p = hough_search_plan(m, n_cu, forced);
  out[0] = p.ok, out[1] = p.lanes, out[2] = p.workgroups;
}
int shim_default_evals() { return HOUGH_SEARCH_EVALS; }
int shim_max_evals() { return (int)HOUGH_SEARCH_MAX_EVALS; }
}
"""

SHAPE = (60, 60)
PC_TRUE = np.array([0.42, 0.22, 0.5])
TOL = float(np.deg2rad(2.0))
TOL_DEG = float(np.degrees(TOL))
N_BANDS = 9


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = str(tmp_path_factory.mktemp("houghsearch"))
    src, lib = os.path.join(tmp, "shim.cpp"), os.path.join(tmp, "libshim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", cases.CSRC, src, "-o", lib], check=True)
    lib = C.CDLL(lib)
    lib.shim_objective.restype = C.c_double
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bands_from_normals(normals, pc=PC_TRUE, shape=SHAPE, n_bands=N_BANDS):
    """(theta, rho) records under `pc` of unit normals in the detector frame: hv_band_normal (csrc/hough_vote.h) inverted."""
    ny, nx = shape
    aspect = nx / ny
    xs, ys = aspect / pc[2] / (nx - 1), 1.0 / pc[2] / (ny - 1)
    xoff, yoff, cx, cy = aspect * pc[0] / pc[2], pc[1] / pc[2], (nx - 1) / 2.0, (ny - 1) / 2.0
    out = np.zeros(n_bands, dtype=_lib.HOUGH_BAND_DTYPE)
    out["a"] = out["k"] = -1
    for i, n in enumerate(np.asarray(normals, dtype=np.float64)):
        c, s = n[0] * xs, -n[1] * ys
        if s < 0 or (s == 0 and c < 0):
            n, c, s = -n, -c, -s
        k = np.hypot(c, s)
        c, s = c / k, s / k
        out["theta"][i] = np.arctan2(s, c)
        out["rho"][i] = c * (xoff / xs - cx) + s * (yoff / ys - cy) - n[2] / k
        out["value"][i], out["valid"][i] = 1.0, 1
    return out


class Problem:
    """One pattern's bands and phase, the shim's objective as a Python callable, and both searches."""

    def __init__(self, shim, bands, phase, s2d):
        self.shim, self.bands = shim, np.ascontiguousarray(bands, dtype=_lib.HOUGH_BAND_DTYPE)
        self.s2d = np.ascontiguousarray(s2d, dtype=np.float64)
        self.normals = np.ascontiguousarray(phase.normals, dtype=np.float64)
        self.family = np.ascontiguousarray(phase.family, dtype=np.int32)
        self.angles = np.ascontiguousarray(phase.angles, dtype=np.float64)
        self.asked = []
        d = C.c_double
        self.table = (C.c_int(SHAPE[0]), C.c_int(SHAPE[1]), ptr(self.s2d), C.c_int(len(self.normals)),
                      C.c_int(int(self.family.max()) + 1), ptr(self.normals), ptr(self.family), ptr(self.angles), d(TOL), d(TOL_DEG))

    def objective(self, pc):
        pc = np.ascontiguousarray(pc, dtype=np.float64)
        self.asked.append(pc.copy())
        return float(self.shim.shim_objective(ptr(self.bands), C.c_int(len(self.bands)), ptr(pc), *self.table))

    def scipy(self, pc0, **options):
        self.asked = []
        return minimize(self.objective, np.asarray(pc0, dtype=np.float64), method="Nelder-Mead", options=options)

    def header(self, pc0, max_evals, xatol=1e-4, fatol=1e-4, maxiter=None, maxfev=None):
        if maxiter is None and maxfev is None:  # SciPy's resolution of the budget (`resolve_budget` in csrc/extras.hip)
            maxiter = maxfev = 600
        elif maxiter is None:
            maxiter = 2**31 - 1
        elif maxfev is None:
            maxfev = 2**31 - 1
        pc0 = np.ascontiguousarray(pc0, dtype=np.float64)
        x, fun, counts = np.zeros(3), C.c_double(0), np.zeros(3, dtype=np.int32)
        calls = self.shim.shim_search(ptr(self.bands), C.c_int(len(self.bands)), *self.table, ptr(pc0), C.c_double(xatol),
                                      C.c_double(fatol), C.c_int(maxiter), C.c_int(maxfev), C.c_int(max_evals), C.c_int(10**6),
                                      ptr(x), C.byref(fun), ptr(counts))
        return calls, x, fun.value, int(counts[0]), int(counts[1]), int(counts[2])


def problems(shim):
    out = {}
    for seed in (7, 11, 23):
        normals, _, phase, s2d = cases.synthetic_normals(seed=seed)
        out[f"seed{seed}"] = Problem(shim, bands_from_normals(normals), phase, s2d)
    empty = bands_from_normals(normals)
    empty["valid"] = 0
    out["no_valid_band"] = Problem(shim, empty, phase, s2d)
    return out


def same(res, got):
    _, x, fun, nfev, nit, status = got
    return (np.array_equal(res.x.view(np.uint64), x.view(np.uint64)) and np.float64(res.fun).tobytes() == np.float64(fun).tobytes()
            and res.nfev == nfev and res.nit == nit and res.status == status)


def test_bands_from_normals_come_back(shim):
    """The helper inverts hv_band_normal: at the true PC every true normal is recovered, and the objective there is small."""
    normals, _, phase, s2d = cases.synthetic_normals()
    p = Problem(shim, bands_from_normals(normals), phase, s2d)
    f_true, f_off = p.objective(PC_TRUE), p.objective(PC_TRUE + [0.03, -0.03, 0.03])
    assert 0 <= f_true < f_off <= TOL_DEG + 1e-12
    # three of the nine bands are outliers: charged the tolerance each
    assert abs(f_true - 3 * TOL_DEG / 9) < 0.05
    assert p.objective([0.4, 0.2, 0.0]) == 180.0 and p.objective([0.4, 0.2, -0.1]) == 180.0 and p.objective([0.4, 0.2, np.nan]) == 180.0


@pytest.mark.parametrize("max_evals", [1, 7, 10**6])
def test_search_is_scipy_bit_for_bit(shim, max_evals):
    pc0 = PC_TRUE + [0.012, -0.008, 0.01]
    for name, p in problems(shim).items():
        res = p.scipy(pc0, xatol=1e-3, fatol=1e-3)
        got = p.header(pc0, max_evals, xatol=1e-3, fatol=1e-3)
        print(name, "max_evals", max_evals, "calls", got[0], "x", got[1], "fun", got[2], "nfev", got[3], "nit", got[4], "status", got[5])
        assert got[0] > 0 and same(res, got), (name, res, got)
        # cut into launches of max_evals: as many calls as that takes
        assert got[0] == (1 if max_evals >= res.nfev else -(-res.nfev // max_evals)) or got[0] == -(-res.nfev // max_evals) + 1
    # a pattern without a valid band: the objective is the tolerance everywhere, the search converges at once
    res = problems(shim)["no_valid_band"].scipy(pc0, xatol=1e-3, fatol=1e-3)
    assert res.fun == TOL_DEG and res.status == 0
    # the real searches moved and found the three outliers' charge
    res = problems(shim)["seed7"].scipy(pc0, xatol=1e-3, fatol=1e-3)
    assert res.nfev > 20 and abs(res.fun - 3 * TOL_DEG / 9) < 0.05 and np.abs(res.x - PC_TRUE).max() < 0.02


@pytest.mark.parametrize("max_evals", [1, 7, 10**6])
def test_simplex_that_crosses_pcz_zero(shim, max_evals):
    """Starts at the screen and behind it: vertices with PCz <= 0 cost 180.  (From PCz = 0.01 these band sets keep the
    simplex in front of the screen; that start is compared all the same.)"""
    p = problems(shim)["seed7"]
    crossed = {}
    for pcz in (0.01, 0.0, -0.01):
        pc0 = [0.42, 0.22, pcz]
        res = p.scipy(pc0, xatol=1e-3, fatol=1e-3)
        crossed[pcz] = sum(not pc[2] > 0 for pc in p.asked)
        assert same(res, p.header(pc0, max_evals, xatol=1e-3, fatol=1e-3)), pcz
    print("evaluations with PCz <= 0:", crossed)
    assert crossed[0.0] >= 3 and crossed[-0.01] >= 4


@pytest.mark.parametrize("max_evals", [1, 7, 10**6])
@pytest.mark.parametrize("budget", [dict(maxfev=5), dict(maxiter=2), dict(maxfev=3), dict(maxiter=40, maxfev=25), dict(maxfev=25)])
def test_budgets_end_where_scipy_ends(shim, budget, max_evals):
    import warnings

    p = problems(shim)["seed11"]
    pc0 = PC_TRUE + [0.012, -0.008, 0.01]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # SciPy warns that the budget ran out
        res = p.scipy(pc0, xatol=1e-3, fatol=1e-3, **budget)
    got = p.header(pc0, max_evals, xatol=1e-3, fatol=1e-3, **budget)
    print(budget, "nfev", res.nfev, "nit", res.nit, "status", res.status)
    assert res.status in (1, 2) and same(res, got), (budget, res, got)


def test_search_plan(shim):
    def plan(m, n_cu, forced=0):
        out = np.zeros(3, dtype=np.int64)
        shim.shim_plan(C.c_int64(m), C.c_int(n_cu), C.c_int(forced), ptr(out))
        return tuple(int(v) for v in out)

    # 256 CUs: a small grid is one lane per workgroup, one workgroup per pattern; a large one fills waves
    assert [plan(m, 256) for m in (1, 63, 64, 65)] == [(1, 1, 1), (1, 1, 63), (1, 1, 64), (1, 1, 65)]
    assert plan(256, 256) == (1, 1, 256) and plan(257, 256) == (1, 2, 129) and plan(64 * 256, 256) == (1, 64, 256)
    assert plan(10**6, 256) == (1, 64, 15625) and plan(10**6 + 1, 256) == (1, 64, 15626)
    # 8 CUs: the lanes double as ceil(m / n_cu) passes a power of two
    assert [plan(m, 8) for m in (1, 63, 64, 65)] == [(1, 1, 1), (1, 8, 8), (1, 8, 8), (1, 16, 5)]
    assert plan(10**6, 8) == (1, 64, 15625)
    # forced lanes (tests), and what is refused
    assert plan(130, 256, 64) == (1, 64, 3) and plan(65, 256, 4) == (1, 4, 17) and plan(3, 256, 64) == (1, 64, 1)
    assert plan(0, 256)[0] == 0 and plan(5, 0)[0] == 0 and plan(5, 256, 65)[0] == 0 and plan(5, 256, -1)[0] == 0
    for m in (1, 63, 64, 65, 10**6):
        for n_cu in (8, 256):
            ok, lanes, groups = plan(m, n_cu)
            assert ok and lanes in (1, 2, 4, 8, 16, 32, 64) and (groups - 1) * lanes < m <= groups * lanes
    assert shim.shim_max_evals() == _lib.HOUGH_SEARCH_MAX_EVALS == 10000
    assert shim.shim_default_evals() == _lib.HOUGH_SEARCH_EVALS == 6 and shim.shim_state_bytes() % 8 == 0



def test_which_keywords_take_the_kernel(monkeypatch):
    """`_device_search_options`: plain keywords give the kernel's options, everything else None (the host loop)."""
    from kikuchipy_amd.indexing._hough_indexing import _device_search_options as parse

    monkeypatch.delenv("KPDI_HOUGH_PC_SEARCH", raising=False)
    assert parse({}) == dict(xatol=1e-3, fatol=1e-3, maxiter=None, maxfev=None)
    assert parse(dict(options=dict(xatol=1e-4, maxfev=25, disp=False), tol=1e-5)) == dict(xatol=1e-4, fatol=1e-3, maxiter=None, maxfev=25)
    assert parse(dict(options=dict(maxiter=1999))) is not None and parse(dict(options=dict(maxfev=_lib.HOUGH_SEARCH_MAX_EVALS))) is not None
    for host in (dict(options=dict(adaptive=True)), dict(bounds=[(0, 1)] * 3), dict(callback=print), dict(options=dict(disp=True)),
                 dict(options=dict(initial_simplex=np.zeros((4, 3)))), dict(options=dict(return_all=True)), dict(options=dict(maxfev=25.0)),
                 dict(options=dict(maxiter=2000)), dict(options=dict(maxfev=_lib.HOUGH_SEARCH_MAX_EVALS + 1)), dict(options=dict(maxfev=0))):
        assert parse(host) is None, host
    monkeypatch.setenv("KPDI_HOUGH_PC_SEARCH", "host")
    assert parse({}) is None
