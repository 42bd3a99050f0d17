"""What `kpdi_plan_describe` says is what the engine launches: both read the one plan::SweepPlan of csrc/plan.h.

Each case of tests/_plan_engine_worker.py is swept once at profiling level 2, in a fresh child process per kernel form
($KPDI_F32_WIDE is read by `kpdi_set_problem`); the counters the engine takes from its plan - `match_form`,
`match_nsplit`, `match_grid` - must be the described form, split and largest padded grid, and the result must be the
brute-force NumPy top-k of the reference's `match` + `topk` (indexing/_dictionary_indexing.py:172-203;
similarity_metrics/_normalized_cross_correlation.py:161-183): indices equal wherever the scores are untied, scores within
the engine tests' 1e-5 (tests/test_gpu_engine.py).  Where both forms sweep the same case they must agree bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _plan_engine_worker as worker
from oracle import kpdi_oracle as ko

pytestmark = pytest.mark.gpu

ATOL = 1e-5
N_CU = 256  # compute units of an MI355X
CASES = [(form, j) for form in sorted(worker.CASES) for j in range(len(worker.CASES[form]))]


RUNS = {}  # form -> what its child process left: the arrays, or why there are none (a failed worker is not run again)


def engine(form, tmp):
    """Everything the worker measured for one kernel form: one child process, shared by the cases of that form."""
    if form not in RUNS:
        path = os.path.join(tmp, f"form{form}.npz")
        env = dict(os.environ, KPDI_F32_WIDE="1" if form == 3 else "0")
        for k in ("KPDI_TAIL_GEMM", "KPDI_NO_TAIL", "KPDI_TILE_ORDER", "KPDI_XCD_GRID", "KPDI_XCD_PAD", "KPDI_ONE_STREAM"):
            env.pop(k, None)
        RUNS[form] = f"worker of form {form} did not finish"
        p = subprocess.run([sys.executable, worker.__file__, str(form), path], env=env, capture_output=True, text=True, timeout=600)
        if p.returncode == 0:
            with np.load(path) as f:
                RUNS[form] = {k: f[k] for k in f.files}
        else:
            RUNS[form] = f"worker of form {form} exited with {p.returncode}: " + p.stdout[-1500:] + p.stderr[-1500:]
    assert isinstance(RUNS[form], dict), RUNS[form]
    return RUNS[form]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("plan_engine"))


@functools.lru_cache(maxsize=None)
def brute_force_topk(m, n, keep_n):
    """Normalised cross-correlation of every pair in float64, the best keep_n per row, ties by rising dictionary index."""
    def unit(a):
        a = a.reshape(len(a), -1).astype(np.float64)
        a -= a.mean(axis=1, keepdims=True)
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    exp, dic = worker.inputs(m, n)
    x, y = unit(exp), unit(dic)
    scores, indices = np.empty((m, keep_n)), np.empty((m, keep_n), dtype=np.int64)
    for r0 in range(0, m, 2048):
        s = x[r0:r0 + 2048] @ y.T
        best = np.argpartition(-s, keep_n - 1, axis=1)[:, :keep_n]
        sb = np.take_along_axis(s, best, 1)
        o = np.lexsort((best, -sb), axis=1)
        scores[r0:r0 + 2048], indices[r0:r0 + 2048] = np.take_along_axis(sb, o, 1), np.take_along_axis(best, o, 1)
    return scores, indices


@pytest.mark.parametrize("form,j", CASES, ids=[f"form{f}-{'x'.join(map(str, worker.CASES[f][j]))}" for f, j in CASES])
def test_engine_launches_the_described_plan(tmp, form, j):
    from kikuchipy_amd import _lib

    m, n, keep_n = worker.CASES[form][j]
    got = engine(form, tmp)
    p = _lib.plan_describe(m, n, worker.SHAPE[0] * worker.SHAPE[1], keep_n, N_CU, form)
    grid = max(p.launch[i].rows_grid for i in range(p.n_launch_desc)) * p.nsplit
    print(f"form {form} m {m} n {n} keep_n {keep_n}: described (form, nsplit, grid) = {(p.form, p.nsplit, grid)}, "
          f"engine = {tuple(got[f'counters__{j}'].tolist())}")
    assert p.launches == p.n_launch_desc  # (every launch of these cases is described)
    assert got[f"counters__{j}"].tolist() == [p.form, p.nsplit, grid]
    s, i = got[f"scores__{j}"], got[f"indices__{j}"]
    assert s.dtype == np.float32 and i.dtype == np.int64 and s.shape == i.shape == (m, keep_n)
    ko.assert_topk_parity(s, i, *brute_force_topk(m, n, keep_n), atol=ATOL)
    other = 3 - form
    if (m, n, keep_n) in worker.CASES[other]:
        o = engine(other, tmp)
        jo = worker.CASES[other].index((m, n, keep_n))
        assert np.array_equal(s.view(np.uint32), o[f"scores__{jo}"].view(np.uint32)) and np.array_equal(i, o[f"indices__{jo}"])
