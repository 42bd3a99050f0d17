"""Time geometrical simulations (`KikuchiPatternSimulator.on_detector`, csrc/geometrical.hip) on a 200 x 200 map with the
Ni reflector list of the kinematical fixtures, and write profiles/geometrical_bench.json:

- `visibility_ms`, `coordinates_ms`: the kernels between events on the library's stream (`geometrical_*_ms` of the
  counters with profiling on; the coordinate kernel summed over its passes; the two visibility calls added up);
- `call_ms`: the whole `on_detector` call, host table, zone-axis reduction and copies included (median of `--repeats`);
- `numpy_ms`: the NumPy restatement of tests/_geometrical_cases.py on `--points` of the map's points, 16 threads;
- `bytes_stored` of the coordinate pass (65 per (point, line), 33 per (point, zone axis)) and the rate it gives against
  the HBM rate of MI355X_MICROARCH (8 TB/s peak).

    python tools/bench_geometrical.py [--side 200] [--repeats 5] [--points 400]"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "16")

HBM_PEAK_BYTES_PER_S = 8.0e12


def main():
    import _geometrical_cases as cases
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=400)
    args = ap.parse_args()
    hkl = cases.ni_hkl()
    rot = cases.random_rotations(1, (args.side, args.side), spread=0.02)  # a map of one grain with some spread
    det = kpa.EBSDDetector(shape=(60, 60), pc=cases.random_pcs(2, (args.side, args.side)), sample_tilt=70.0)
    simulator = kpa.KikuchiPatternSimulator(kpa.Reflectors(hkl, None, phase_name="ni"))
    with _lib.Context(0) as ctx:
        sim = simulator.on_detector(det, rot, context=ctx)  # warm-up
        ctx.set_profiling(1)
        vis = ctx.geometrical_visibility
        vis_ms = []

        def timed_visibility(*a, **k):
            out = vis(*a, **k)
            vis_ms[-1] += ctx.counters()["geometrical_visibility_ms"]
            return out

        ctx.geometrical_visibility = timed_visibility
        call, coord = [], []
        for _ in range(args.repeats):
            vis_ms.append(0.0)
            t = time.perf_counter()
            sim = simulator.on_detector(det, rot, context=ctx)
            call.append((time.perf_counter() - t) * 1e3)
            coord.append(ctx.counters()["geometrical_coordinates_ms"])
    n, m, z = args.side**2, sim.reflectors.size, sim.zone_axes.shape[0]
    stored = n * (m * 65 + z * 33)
    case = {"name": "bench", "hkl": hkl, "basis": np.eye(3), "rotations": rot.reshape(-1, 4)[:args.points],
            "pc": det.pc.reshape(-1, 3)[:args.points], "det": dict(shape=(60, 60), sample_tilt=70.0), "exact": False}
    t = time.perf_counter()
    cases.simulate(case)
    numpy_ms = (time.perf_counter() - t) * 1e3
    coord_ms = float(np.median(coord))
    out = {"map": [args.side, args.side], "reflectors": int(hkl.shape[0]), "lines_kept": int(m), "zone_axes_kept": int(z),
           "visibility_ms": float(np.median(vis_ms)), "coordinates_ms": coord_ms, "call_ms": float(np.median(call)),
           "numpy_points": args.points, "numpy_ms": numpy_ms, "numpy_ms_scaled_to_map": numpy_ms * n / args.points,
           "bytes_stored": int(stored), "store_rate_bytes_per_s": stored / (coord_ms * 1e-3),
           "share_of_hbm_peak": stored / (coord_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, "library": _lib.version()}
    path = os.path.join(ROOT, "profiles", "geometrical_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
