"""SciPy's Nelder-Mead without a GPU: csrc/nelder_mead.h compiled with the host compiler and run over
tests/_nelder_mead_cases.py against `scipy.optimize.minimize(method="Nelder-Mead")` bit for bit, with every branch of the
header reached."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import _nelder_mead_cases as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The objectives are csrc/analytic_objectives.h; their independent statement is tests/_powell_cases.py, which SciPy runs.
# One line per case on stdin:
#   kind n bounded xatol fatol maxiter maxfev x0[n] [lower[n] upper[n]]     (floats as C99 hex, 0 = limit not set)
# one line per case out: nfev nit fun x[n] (floats as their 64 bits), then "count <name> <hits>" per branch.
# The budget is resolved as `resolve_budget` (csrc/extras.hip) does: both unset = 200 n each, one unset = that one
# unlimited.
DRIVER = r"""
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "analytic_objectives.h"
#include "nelder_mead.h"

static unsigned long long bits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, 8);
  return u;
}

int main() {
  char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    char *p = line;
    kpdi::AnalyticObjective f;
    f.kind = (int)std::strtol(p, &p, 10);
    f.n = (int)std::strtol(p, &p, 10);
    const int bounded = (int)std::strtol(p, &p, 10);
    const double xatol = std::strtod(p, &p), fatol = std::strtod(p, &p);
    int maxiter = (int)std::strtol(p, &p, 10), maxfev = (int)std::strtol(p, &p, 10);
    double x0[6], lo[6], hi[6];
    if (f.kind < 0 || f.kind > 4 || f.n < 1 || f.n > 6) return 2;
    for (int i = 0; i < f.n; ++i) x0[i] = std::strtod(p, &p);
    if (bounded) {
      for (int i = 0; i < f.n; ++i) lo[i] = std::strtod(p, &p);
      for (int i = 0; i < f.n; ++i) hi[i] = std::strtod(p, &p);
    }
    const bool no_it = maxiter <= 0, no_fev = maxfev <= 0;
    if (no_it && no_fev) maxiter = maxfev = f.n * 200;
    else if (no_it) maxiter = INT_MAX;
    else if (no_fev) maxfev = INT_MAX;
    static kpdi::NelderMead<6> s;
    s.begin(f.n, x0, bounded ? lo : nullptr, bounded ? hi : nullptr, xatol, fatol, maxiter, maxfev);
    while (s.state != kpdi::NelderMead<6>::S_DONE) s.feed(f.eval(s.xeval));
    std::printf("%d %d %016llx", s.fcalls, s.iterations, bits(s.fun()));
    for (int i = 0; i < f.n; ++i) std::printf(" %016llx", bits(s.sim[0][i]));
    std::printf("\n");
  }
  for (int b = 0; b < kpdi::NMB_COUNT; ++b)
    std::printf("count %s %lld\n", kpdi::kpdi_nelder_mead_branch_names[b], kpdi::kpdi_nelder_mead_count[b]);
  return 0;
}
"""

# Branches of nelder_mead.h that no case reaches, with the reason (at most three may be listed).
UNREACHED = {
    "bg_first_raise": "the first evaluation raises only with a budget below 1, and the resolved budget is at least 1: a "
                      "limit of 0 or less means `not set`, as in `resolve_budget`",
    "lt_reflect_raise": "the loop's condition has just found fcalls < maxfun when the reflected point is requested",
}


def case_line(case):
    kind, x0, bounds, opt = case
    words = [str(kind), str(len(x0)), "0" if bounds is None else "1", float(opt.get("xatol", 1e-4)).hex(),
             float(opt.get("fatol", 1e-4)).hex(), str(opt.get("maxiter", 0)), str(opt.get("maxfev", 0))]
    words += [float(v).hex() for v in x0]
    if bounds is not None:
        words += [float(v).hex() for v in bounds[0]] + [float(v).hex() for v in bounds[1]]
    return " ".join(words)


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("nelder_mead")
    src, exe = tmp / "nelder_mead_driver.cpp", tmp / "nelder_mead_driver"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-DKPDI_NELDER_MEAD_COUNT", "-I",
                    os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    text = "\n".join(case_line(c) for c in nm.CASES) + "\n"
    out = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.strip().split("\n")
    rows = [ln.split() for ln in out if not ln.startswith("count ")]
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in out if ln.startswith("count ")}
    assert len(rows) == len(nm.CASES)
    return rows, counts


def from_bits(words):
    return np.array([int(w, 16) for w in words], dtype=np.uint64).view(np.float64)


@pytest.mark.parametrize("case", range(len(nm.CASES)))
def test_header_matches_scipy_bit_for_bit(driver_output, case):
    row = driver_output[0][case]
    want = nm.want(case)
    nfev, nit = int(row[0]), int(row[1])
    fun, x = from_bits(row[2:3])[0], from_bits(row[3:])
    print(nm.CASES[case], "header", nfev, nit, fun, x, "scipy", want.nfev, want.nit, want.fun, want.x)
    assert (nfev, nit) == (want.nfev, want.nit), (row, want)
    assert nm.same_bits(x, want.x), (x, want.x)
    assert nm.same_bits(fun, want.fun), (fun, want.fun)


def test_the_table_covers_what_it_is_there_for():
    cases = nm.CASES
    assert {len(c[1]) for c in cases} >= {1, 2, 3, 6} and {c[0] for c in cases} == {0, 1, 2, 3, 4}
    assert any(c[0] == 3 and c[1][0] == 1.85 for c in cases) and any(c[0] == 3 and c[1][0] > 1.9 for c in cases)
    assert any(c[0] == 2 and c[3].get("xatol") == 1e-12 == c[3].get("fatol") for c in cases)
    assert any(c[2] is not None and np.any(np.equal(*c[2])) for c in cases)                     # lower == upper
    assert any(c[2] is not None and np.any(np.equal(c[1], c[2][0]) | np.equal(c[1], c[2][1])) for c in cases)
    # every value NaN: SciPy's termination test is false, the search uses up its budget of 200 n
    for i, c in enumerate(cases):
        if c[0] == 4 and not c[3]:
            assert nm.want(i).nfev == 200 * len(c[1]) and np.isnan(nm.want(i).fun)
    assert max(nm.want(i).nfev for i in range(len(cases))) <= 1200


def test_every_branch_of_the_header_is_reached(driver_output):
    counts = driver_output[1]
    assert len(UNREACHED) <= 3 and set(UNREACHED) <= set(counts)
    missed = sorted(name for name, hits in counts.items() if hits == 0 and name not in UNREACHED)
    assert not missed, missed
    assert all(counts[name] == 0 for name in UNREACHED), "a branch listed as unreachable was reached: take it off the list"
