"""One table of differential-evolution cases for the host test (csrc/differential_evolution.h compiled with the host
compiler) and the GPU test (`kpdi_de_selftest`), with the analytic objectives in the operation order of the C++ ones
(`AnalyticObjective` in csrc/analytic_objectives.h, kinds numbered through `analytic_kind_de`): each row runs through
`scipy.optimize.differential_evolution(fun, bounds, polish=False, **kw)` and through the restatement, and the two must
agree bit for bit.  Also the programs of random draws both tests run against `numpy.random.RandomState`."""

import numpy as np
import scipy.optimize

import _powell_cases as pc

DE_POP_MAX = 256  # KPDI_DE_POP_MAX of include/kpdi.h


def hug(x):
    """Minimum on the lower bound of a box that starts at 0: trial vectors leave [0, 1] and are drawn again."""
    acc = None
    for i in range(len(x)):
        d = abs(x[i])
        t = float(i + 1) * (d * d + 0.1 * d)
        acc = t if acc is None else acc + t
    return float(acc)


def all_inf(x):
    return float("inf")


def constant(x):
    return 0.1


# kinds 0..4: those of kpdi_powell_selftest; 5: hug; 6: +inf everywhere; 7: 0.1 everywhere
OBJECTIVES = pc.OBJECTIVES + (hug, all_inf, constant)

same_bits = pc.same_bits


def box(n, lo, hi):
    return [float(lo)] * n, [float(hi)] * n


# kind, (lower, upper), keyword arguments of differential_evolution, what SciPy 1.15.3 returns where pinned
# (members = the population SciPy works out; the premises are asserted in tests/test_host_de.py)
CASES = [
    # the defaults of the refinement: 45 members for three variables, 90 for six
    (1, box(3, -1, 2), dict(seed=1, maxiter=30), dict(members=45, nit=30, success=False)),
    (1, box(6, -1, 2.5), dict(seed=2, maxiter=8), dict(members=90, nit=8, success=False)),
    (0, box(2, -2, 2), dict(seed=3, popsize=4, maxiter=40, updating="deferred"), dict(members=8)),
    (1, box(1, -1, 2), dict(seed=0, maxiter=60), dict(members=15, success=True)),
    (1, box(1, -1, 2), dict(seed=4, popsize=7, maxiter=20, updating="deferred", init="random"), dict(members=7)),
    (1, box(3, -1, 2), dict(seed=5, popsize=1, maxiter=25), dict(members=5)),
    (0, box(3, 0.5, 1.5), dict(seed=6, popsize=3, maxiter=30, init="random"), dict(members=9)),
    (1, box(4, -1, 2), dict(seed=7, popsize=2, maxiter=30, updating="deferred", mutation=0.8, recombination=1),
     dict(members=8)),
    (1, box(5, -1, 2), dict(seed=8, popsize=5, maxiter=20, init="random", updating="deferred", mutation=(0.3, 1.2)),
     dict(members=25)),
    (1, box(6, -1, 2.5), dict(seed=9, popsize=4, maxiter=15, mutation=0.6, recombination=0), dict(members=24)),
    (0, box(2, -2, 2), dict(seed=10, popsize=6, maxiter=12, mutation=(1.0, 0.4), recombination=1.0), dict(members=12)),
    # the pairwise-sum boundaries above 128 members, and the cap
    (2, box(3, -1, 2), dict(seed=11, popsize=43, maxiter=4), dict(members=129)),
    (2, box(1, -1, 2), dict(seed=12, popsize=129, maxiter=4, updating="deferred"), dict(members=129)),
    (1, box(4, -1, 2), dict(seed=13, popsize=64, maxiter=3, updating="deferred"), dict(members=DE_POP_MAX)),
    (2, box(2, -1, 2), dict(seed=14, popsize=128, maxiter=3, init="random"), dict(members=DE_POP_MAX)),
    # tol = atol = 0: only an exactly constant population would converge; ends by maxiter
    (0, box(3, 0.5, 1.5), dict(seed=15, popsize=3, maxiter=5, tol=0, atol=0), dict(members=9, nit=5, success=False)),
    # a constant objective converges after the first generation, in both modes; every trial ties with its candidate
    (7, box(3, -1, 2), dict(seed=16, popsize=3, maxiter=9), dict(members=9, nit=1, success=True)),
    (7, box(2, -1, 2), dict(seed=17, popsize=4, maxiter=9, updating="deferred"), dict(members=8, nit=1, success=True)),
    # tol = atol = 0 on equal energies hangs on the summation order: numpy's pairwise mean of 45 times 0.1 is not 0.1
    # (a plain sum's is), so np.std is 4e-17 and nothing converges; of 9 times 0.1 it is 0.1 (a plain sum's is not)
    (7, box(3, -1, 2), dict(seed=18, maxiter=3, tol=0, atol=0), dict(members=45, nit=3, success=False)),
    # convergence in the last generation allowed (maxiter = the generation the search converges in)
    (1, box(3, -1, 2), dict(seed=1, maxiter=None), dict(members=45, success=True, last=True)),
    (1, box(2, -1, 2), dict(seed=19, popsize=5, maxiter=None, updating="deferred", atol=1e-3),
     dict(members=10, success=True, last=True)),
    # the minimum on the bounds: _ensure_constraint draws again
    (5, box(3, 0, 1.5), dict(seed=20, popsize=5, maxiter=25), dict(members=15, redraws=True)),
    (5, box(6, 0, 1.5), dict(seed=21, popsize=3, maxiter=12, updating="deferred", mutation=(0.5, 1.9)),
     dict(members=18, redraws=True)),
    (5, box(1, 0, 1.5), dict(seed=22, popsize=9, maxiter=12, updating="deferred", init="random"),
     dict(members=9, redraws=True)),
    # a held variable (lower == upper): it does not count for the population
    (1, ([-1.0, 0.6, -1.0], [2.0, 0.6, 2.0]), dict(seed=23, maxiter=20), dict(members=30)),
    (1, ([0.3, 0.6, 0.9], [0.3, 0.6, 0.9]), dict(seed=24, maxiter=3, updating="deferred"), dict(members=15, nit=1)),
    # NaN somewhere and everywhere; +inf everywhere (the energies are worked out again in every generation)
    (3, ([0.5, 0.0, 0.0], [2.05, 1.5, 0.6]), dict(seed=25, popsize=5, maxiter=6), dict(members=15)),
    (3, ([0.5, 0.0, 0.0], [2.05, 1.5, 0.6]), dict(seed=26, popsize=5, maxiter=6, updating="deferred"), dict(members=15)),
    (4, box(3, -1, 2), dict(seed=27, popsize=2, maxiter=3), dict(members=6, nit=3, success=False)),
    (4, box(2, -1, 2), dict(seed=28, popsize=3, maxiter=2, updating="deferred"), dict(members=6, nit=2, success=False)),
    (6, box(3, -1, 2), dict(seed=29, popsize=2, maxiter=2), dict(members=6, nit=2, nfev=30, success=False)),
    (6, box(2, -1, 2), dict(seed=30, popsize=3, maxiter=2, updating="deferred"), dict(members=6, nit=2, nfev=30)),
    (7, box(3, -1, 2), dict(seed=31, popsize=3, maxiter=3, tol=0, atol=0), dict(members=9, nit=1, success=True)),
    # the largest seed, no generation at all
    (1, box(3, -1, 2), dict(seed=2**32 - 1, popsize=3, maxiter=0), dict(members=9, nit=0, nfev=9, success=False)),
]

# the cases the GPU test runs: one and six variables, both updating modes, both initialisations, the redraws, the cap
GPU_CASES = [1, 2, 3, 4, 8, 13, 17, 21, 22, 25, 27, 32, 33]


def members(case):
    """num_population_members as SciPy works it out (_differentialevolution.py:925-928)."""
    lower, upper = np.asarray(case[1][0]), np.asarray(case[1][1])
    popsize = case[2].get("popsize", 15)
    return max(5, popsize * max(1, lower.size - int(np.count_nonzero(lower == upper))))


def mutation_pair(mutation):
    """(lo, hi) as the C entry points take `mutation`: hi = NaN for a float, else SciPy's sorted dither pair."""
    if np.ndim(mutation) == 0:
        return float(mutation), float("nan")
    lo, hi = sorted(float(m) for m in mutation)
    return lo, hi


def scipy_run(case, maxiter):
    kind, (lower, upper), kw, _ = case
    kw = dict(kw, maxiter=maxiter)
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # NaN energies
        return scipy.optimize.differential_evolution(OBJECTIVES[kind], list(zip(lower, upper)), polish=False, **kw)


_WANT = {}


def want(i):
    """SciPy's result of case i and the maxiter it ran with, computed once.  `maxiter=None` in the table: the
    generation in which SciPy's own default run converges."""
    if i not in _WANT:
        case = CASES[i]
        maxiter = case[2]["maxiter"]
        if maxiter is None:
            maxiter = scipy_run(case, 1000).nit
        _WANT[i] = scipy_run(case, maxiter), maxiter
    return _WANT[i]


# ---- programs of draws: rows (op, a, b) - 0: uniform(), 1: uniform(a, b), 2: randint(0, a), 3: shuffle of the
# persistent arange(a), 4: permutation(range(a))
def _mixed(n_rows, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_rows):
        op = int(rng.integers(0, 5))
        if op == 1:
            a = float(rng.uniform(-3, 3))
            rows.append((1, a, a + float(rng.uniform(0, 5))))
        elif op == 2:
            rows.append((2, int(rng.integers(1, 7)), 0))
        elif op >= 3:
            rows.append((op, int(rng.choice([5, 8, 9, 45])), 0))
        else:
            rows.append((0, 0, 0))
    return rows


PROGRAMS = [
    (0, [(0, 0, 0)] * 400),                                                     # 800 words: the twist runs
    (1, [(2, n, 0) for n in (1, 2, 3, 4, 5, 6)] * 40),
    (2**32 - 1, [(3, s, 0) for s in (5, 8, 9, 45, 90, 128, 129, DE_POP_MAX)] * 2),  # masks on both sides of a power of two
    (12345, [(4, s, 0) for s in (5, 8, 9, 45, 90, 128, 129, DE_POP_MAX)]),
    (987654321, [(1, 0.5, 1.0), (1, -2.0, 3.5), (1, 0.0, 1.9)] * 30),
    (7, _mixed(300, 7)),
    (2024, _mixed(300, 8)),
]
GPU_PROGRAMS = [0, 2, 5]


def program_array(rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def program_words(rows):
    return sum(int(a) if op >= 3 else 1 for op, a, _ in rows)


def program_want(seed, rows):
    """The 64-bit words the draws of `rows` return from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    out, index = [], np.arange(0)
    for op, a, b in rows:
        if op == 0:
            out.append(np.float64(rs.uniform()).view(np.uint64))
        elif op == 1:
            out.append(np.float64(rs.uniform(a, b)).view(np.uint64))
        elif op == 2:
            out.append(np.uint64(rs.randint(0, int(a))))
        elif op == 3:
            if index.size != int(a):
                index = np.arange(int(a))
            rs.shuffle(index)
            out.extend(index.astype(np.uint64))
        else:
            out.extend(rs.permutation(range(int(a))).astype(np.uint64))
    return np.array(out, dtype=np.uint64)
