"""Time `refine_orientation(method="basinhopping", method_kwargs=dict(minimizer_kwargs=dict(method="Nelder-Mead")))` -
SciPy's defaults: 100 hops, each a full Nelder-Mead quench - on a resident 32 x 32 map of 60 x 60 patterns, on the
device path (`kpdi_refine_solve_basinhopping`: one launch) and on the host path (KPDI_REFINE_BASINHOPPING=host: SciPy in
Python, one objective launch and one synchronisation per evaluation, one pattern after the other - the only path there
was before the device solver), and write profiles/refine_basinhopping_bench.json.

Both paths are timed once.  The host path needs about 10^4 round trips per pattern, so it is timed on the first
`--host-patterns` points of the map only (a navigation mask hides the rest) and its time for the whole map is that
time scaled by the number of points: `host_wall_s_whole_map_scaled` is arithmetic, not a measurement.  `wall_s`: the
whole call (pattern preparation included); `refine_ms`: the solve kernel between events on the library's stream (device
path only); `evaluations_per_pattern`: mean of `num_evals`.  Every job starts from RandomState(--seed), so the two
paths walk the same searches.

    python tools/bench_refine_basinhopping.py [--host-patterns 8] [--seed 0]"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAV, SIG = (32, 32), (60, 60)


def synthetic_map():
    """A smooth random master pattern, 1024 patterns projected from it on the device with noise added, and starts up to
    a degree off in every Euler angle."""
    import kikuchipy_amd as kpa
    from kikuchipy_amd.indexing._refinement import rotation_from_euler

    rng = np.random.default_rng(99)
    f = np.fft.rfft2(rng.standard_normal((201, 201)))
    ky, kx = np.meshgrid(np.fft.fftfreq(201), np.fft.rfftfreq(201), indexing="ij")
    mpd = np.fft.irfft2(f * np.exp(-(kx**2 + ky**2) / (2 * 0.04**2)), s=(201, 201)).astype(np.float32)
    mp = kpa.EBSDMasterPattern(np.stack([mpd, mpd]), hemisphere="both")
    det = kpa.EBSDDetector(shape=SIG, pc=(0.45, 0.7, 0.55), sample_tilt=70.0)
    n = NAV[0] * NAV[1]
    eu = np.column_stack([rng.uniform(0.3, 6, n), rng.uniform(0.3, 2.8, n), rng.uniform(0.3, 6, n)])
    sim = np.asarray(mp.get_patterns(rotation_from_euler(eu), det).data.compute(), dtype=np.float32).reshape(n, *SIG)
    noisy = sim + 0.3 * sim.std() * rng.standard_normal(sim.shape).astype(np.float32)
    pats = ((noisy - noisy.min()) / (noisy.max() - noisy.min()) * 255).astype(np.uint8).reshape(NAV + SIG)
    eu0 = eu + np.deg2rad(rng.uniform(-1, 1, eu.shape))
    return pats, rotation_from_euler(eu0).reshape(NAV + (4,)), mp, det


def main():
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--host-patterns", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    pats, rot, mp, det = synthetic_map()
    n = NAV[0] * NAV[1]
    s = kpa.EBSD(pats).to_device()
    assert s.is_resident
    kw = dict(method="basinhopping", method_kwargs=dict(seed=args.seed, minimizer_kwargs=dict(method="Nelder-Mead")),
              verbose=False)

    def run(path, navigation_mask=None):
        if path == "host":
            os.environ["KPDI_REFINE_BASINHOPPING"] = "host"
        else:
            os.environ.pop("KPDI_REFINE_BASINHOPPING", None)
        before = s.context.counters()["refine_ms"]
        t = time.perf_counter()
        res = s.refine_orientation(rot, det, mp, navigation_mask=navigation_mask, **kw)
        wall = time.perf_counter() - t
        return wall, s.context.counters()["refine_ms"] - before, res

    hidden = np.ones(n, dtype=bool)
    hidden[:args.host_patterns] = False
    hidden = hidden.reshape(NAV)
    s.refine_orientation(rot, det, mp, navigation_mask=hidden, method="minimize", verbose=False)  # warm-up: context, upload
    device_wall, device_ms, device = run("device")
    host_wall, _, host = run("host", hidden)
    os.environ.pop("KPDI_REFINE_BASINHOPPING", None)
    same = bool(np.array_equal(device.scores[:args.host_patterns], host.scores) and
                np.array_equal(device.num_evals[:args.host_patterns], host.num_evals))
    out = {"map": list(NAV), "detector": list(SIG), "patterns": n, "seed": args.seed,
           "method_kwargs": "niter=100 and every other default, minimizer_kwargs=dict(method='Nelder-Mead')",
           "device_wall_s": device_wall, "device_refine_ms": device_ms, "device_patterns_per_s": n / device_wall,
           "host_patterns": args.host_patterns, "host_wall_s": host_wall,
           "host_patterns_per_s": args.host_patterns / host_wall,
           "host_wall_s_whole_map_scaled": host_wall / args.host_patterns * n,
           "evaluations_per_pattern": {"device": float(np.mean(device.num_evals)), "host": float(np.mean(host.num_evals))},
           "mean_score": {"device": float(np.mean(device.scores)), "host": float(np.mean(host.scores))},
           "host_points_equal_device_points": same, "library": _lib.version()}
    with open(os.path.join(ROOT, "profiles", "refine_basinhopping_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
