"""Time the projection-centre refinement of the reference's pattern-matching tutorial,
`refine_projection_center(method_kwargs=dict(method="Powell", tol=1e-3), trust_region=[0.02] * 3)`, on the device path
(`kpdi_refine_solve_powell`: one launch) and on the host path (KPDI_REFINE_POWELL=host: SciPy in Python, one objective
launch and one synchronisation per evaluation), alternately in one process, and write profiles/refine_powell_bench.json.

The patterns are the 48 synthetic 40 x 40 experiments of `test_many_patterns_against_the_scipy_loop`
(tests/test_gpu_refinement.py), built by the same recipe.  `wall_ms`: the whole call (pattern upload and preparation
included); `refine_ms`: the solve kernel between events on the library's stream (device path only - the host path
launches no solve kernel); `evaluations_per_pattern`: mean of `num_evals`.

    python tools/bench_refine_powell.py [--repeats 3]"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_experiments():
    from kikuchipy_amd.indexing._refinement import rotation_from_euler
    from oracle import kpdi_oracle as ko

    rng = np.random.default_rng(99)
    f = np.fft.rfft2(rng.standard_normal((201, 201)))
    ky, kx = np.meshgrid(np.fft.fftfreq(201), np.fft.rfftfreq(201), indexing="ij")
    mpd = np.fft.irfft2(f * np.exp(-(kx**2 + ky**2) / (2 * 0.04**2)), s=(201, 201)).astype(np.float32)
    n, shape, pc = 48, (40, 40), np.array([0.45, 0.7, 0.55])
    dc = ko.detector_direction_cosines(shape, pc)
    eu = np.column_stack([rng.uniform(0.3, 6, n), rng.uniform(0.3, 2.8, n), rng.uniform(0.3, 6, n)])
    sim = ko.project_patterns(rotation_from_euler(eu), dc, mpd, mpd)
    noisy = sim + 0.3 * sim.std() * rng.standard_normal(sim.shape).astype(np.float32)
    pats = ((noisy - noisy.min()) / (noisy.max() - noisy.min()) * 255).astype(np.uint8).reshape(n, *shape)
    eu0 = eu + np.deg2rad(rng.uniform(-1, 1, eu.shape))
    return pats, rotation_from_euler(eu0), mpd, pc


def main():
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib
    from kikuchipy_amd.indexing import _refinement as rf

    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    pats, rot, mpd, pc = synthetic_experiments()
    det = kpa.EBSDDetector(shape=pats.shape[1:], pc=tuple(pc), sample_tilt=70.0)
    mp = kpa.EBSDMasterPattern(np.stack([mpd, mpd]), hemisphere="both")
    # a start 0.01 off in every PC component, inside the trust region of the call
    start = det.deepcopy()
    start.pc = det.pc + np.array([0.01, -0.01, 0.01])
    wall = {"device": [], "host": []}
    kernel_ms, evals, scores = [], {}, {}
    with _lib.Context(0) as ctx:
        def run(path):
            if path == "host":
                os.environ["KPDI_REFINE_POWELL"] = "host"
            else:
                os.environ.pop("KPDI_REFINE_POWELL", None)
            before = ctx.counters()["refine_ms"]
            t = time.perf_counter()
            res, new_det = rf.refine("pc", pats, rot, start, mp, method_kwargs=dict(method="Powell", tol=1e-3),
                                     trust_region=[0.02] * 3, context=ctx, verbose=False)
            ms = (time.perf_counter() - t) * 1e3
            return ms, ctx.counters()["refine_ms"] - before, res

        run("device")  # warm-up of both paths
        run("host")
        for _ in range(args.repeats):
            for path in ("device", "host"):
                ms, solve_ms, res = run(path)
                wall[path].append(ms)
                evals[path] = float(np.mean(res.num_evals))
                scores[path] = float(np.mean(res.scores))
                if path == "device":
                    kernel_ms.append(solve_ms)
        os.environ.pop("KPDI_REFINE_POWELL", None)
    out = {"patterns": int(pats.shape[0]), "detector": list(pats.shape[1:]), "repeats": args.repeats,
           "device_wall_ms": wall["device"], "host_wall_ms": wall["host"],
           "device_wall_ms_median": float(np.median(wall["device"])), "host_wall_ms_median": float(np.median(wall["host"])),
           "device_refine_ms_median": float(np.median(kernel_ms)),
           "evaluations_per_pattern": evals, "mean_score": scores, "library": _lib.version()}
    with open(os.path.join(ROOT, "profiles", "refine_powell_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
