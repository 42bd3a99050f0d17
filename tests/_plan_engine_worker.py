"""Worker of tests/test_gpu_plan_matches_engine.py: the f32 sweeps of CASES[form] on GPU 0 with the kernel form forced
through $KPDI_F32_WIDE - the switch is read by `kpdi_set_problem` and fixed for the process by the caller, so each
setting gets a fresh process.  Profiling level 2; per case the scores, the indices and the three plan counters go into
the .npz named on the command line:

    KPDI_F32_WIDE=1 python tests/_plan_engine_worker.py 3 out.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE = (8, 8)  # uint8 patterns, experimental and dictionary alike
# form -> (m, n, keep_n).  The first rows are the cases the sweep-plan refactor was specified with (two row blocks: every
# dictionary tile gets a workgroup of its own); the others are the smallest shapes at which the plan takes its other
# turns (tests/test_planner.py covers the turns themselves on the CPU).
CASES = {
    0: [(257, 12500, 20),    # two row blocks, one launch
        (257, 12500, 40),    # keep_n > 32: bounded passes
        (1025, 6600, 20),    # 6 whole rounds of 8 splits + match.hip's quarter-tile tail launch over the last 4 tiles
        (1025, 6600, 40),    # ... bounded passes: no tail launch
        (40000, 300, 20)],   # 157 row blocks = 85 + 72: two launches on two streams
    3: [(257, 12500, 20),
        (257, 1000, 20),     # 4 tiles on a 2 x 4 XCD grid
        (257, 12500, 40),
        (8300, 700, 20),     # 33 row blocks x 3 tiles, one launch
        (2049, 7200, 20),    # 9 row blocks on a padded grid; the last partial round goes to tailgemm.hip
        (2049, 8900, 20),    # ... stays inside the kernel as partial units
        (2049, 8200, 40),    # bounded passes: partial units, never tailgemm.hip
        (40000, 2500, 20)],  # two launches on two streams, permuted tile order, partial units, a padded last grid
}


def inputs(m, n):
    rng = np.random.default_rng(1000 * m + n)
    return rng.integers(0, 256, (m,) + SHAPE, dtype=np.uint8), rng.integers(0, 256, (n,) + SHAPE, dtype=np.uint8)


def main(form, path):
    sys.path.insert(0, ROOT)
    from kikuchipy_amd import _lib

    out = {}
    with _lib.Context(0) as c:
        c.set_profiling("match")
        for j, (m, n, keep_n) in enumerate(CASES[form]):
            exp, dic = inputs(m, n)
            c.set_problem(SHAPE[0], SHAPE[1], None, _lib.METRIC_NCC, keep_n)
            c.set_experimental(exp)
            c.reset_counters()
            # (from device memory: a host chunk may be cut into upload pieces, each planned on its own)
            d_dic = c.dev_alloc(dic.nbytes)
            try:
                c.h2d(d_dic, dic)
                c.push_dictionary_chunk_dev(d_dic, dic.dtype, n, 0)
                out[f"scores__{j}"], out[f"indices__{j}"] = c.finalize(keep_n)
            finally:
                c.dev_free(d_dic)
            cnt = c.counters()
            out[f"counters__{j}"] = np.array([cnt["match_form"], cnt["match_nsplit"], cnt["match_grid"]])
    np.savez(path, **out)


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
