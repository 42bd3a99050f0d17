"""Time the combined orientation and projection-centre refinement of the reference's tutorials,
`refine_orientation_projection_center(method="LN_NELDERMEAD", initial_step=[0.1, 0.05], rtol=1e-3)`, on the device
(`kpdi_refine_solve_nlopt`: one launch), next to the yardstick - the device's SciPy Nelder-Mead (`method="minimize"`,
`kpdi_refine_solve`) on the same patterns from the same starts - alternately in one process, and write
profiles/refine_nlopt_bench.json.

The two searches stop on different criteria (a relative tolerance on f here; absolute tolerances on x and f there), so
patterns/s are reported WITH the evaluations per pattern and the mean score beside them; nothing is asserted.

The patterns are the 48 synthetic 40 x 40 experiments of tools/bench_refine_powell.py.  `wall_ms`: the whole call
(pattern upload and preparation included); `refine_ms`: the solve kernel between events on the library's stream;
`evaluations_per_pattern`: mean of `num_evals`.

    python tools/bench_refine_nlopt.py [--repeats 5] [--out FILE]"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CALLS = {
    "ln_neldermead": dict(method="LN_NELDERMEAD", initial_step=[0.1, 0.05], rtol=1e-3),
    "minimize": dict(method="minimize"),
}


def main():
    import kikuchipy_amd as kpa
    from bench_refine_powell import synthetic_experiments
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing import _refinement as rf

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_nlopt_bench.json"))
    args = ap.parse_args()
    os.environ.pop("KPDI_REFINE_NLOPT", None)
    pats, rot, mpd, pc = synthetic_experiments()
    det = kpa.EBSDDetector(shape=pats.shape[1:], pc=tuple(pc), sample_tilt=70.0)
    mp = kpa.EBSDMasterPattern(np.stack([mpd, mpd]), hemisphere="both")
    # a start 0.01 off in every PC component, as in tools/bench_refine_powell.py
    start = det.deepcopy()
    start.pc = det.pc + np.array([0.01, -0.01, 0.01])
    wall = {name: [] for name in CALLS}
    kernel = {name: [] for name in CALLS}
    evals, scores = {}, {}
    with _lib.Context(0) as ctx:
        def run(name):
            before = ctx.counters()["refine_ms"]
            t = time.perf_counter()
            res, _ = rf.refine("ori_pc", pats, rot, start, mp, context=ctx, verbose=False, **CALLS[name])
            ms = (time.perf_counter() - t) * 1e3
            return ms, ctx.counters()["refine_ms"] - before, res

        for name in CALLS:  # warm-up
            run(name)
        for _ in range(args.repeats):
            for name in CALLS:
                ms, solve_ms, res = run(name)
                wall[name].append(ms)
                kernel[name].append(solve_ms)
                evals[name] = float(np.mean(res.num_evals))
                scores[name] = float(np.mean(res.scores))
    n = int(pats.shape[0])
    out = {"patterns": n, "detector": list(pats.shape[1:]), "repeats": args.repeats, "calls": CALLS,
           "wall_ms": wall, "refine_ms": kernel,
           "wall_ms_median": {k: float(np.median(v)) for k, v in wall.items()},
           "refine_ms_median": {k: float(np.median(v)) for k, v in kernel.items()},
           "patterns_per_second": {k: n / (float(np.median(v)) * 1e-3) for k, v in wall.items()},
           "evaluations_per_pattern": evals, "mean_score": scores, "library": _lib.version()}
    out["patterns_per_second_ratio"] = out["patterns_per_second"]["ln_neldermead"] / out["patterns_per_second"]["minimize"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
