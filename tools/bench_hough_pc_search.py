"""The projection-centre search of `EBSD.hough_indexing_optimize_pc(batch=True)` on one GPU (csrc/hough_search.h; DESIGN.md
section 28): a resident `--grid` x `--grid` grid (10) of 60 x 60 patterns simulated from tests/golden/projection.npz with
true PCs on a plane, every search started from their mean.  Prints one JSON line and writes it to `--out`
(profiles/hough_pc_search.json).

Host-clock times, in the same run, each call ending with its results on the host:
- `device_ms`: the whole call on the device path (band detection included), best of `--reps` warm calls;
- `host_ms`: the same call under KPDI_HOUGH_PC_SEARCH=host - SciPy on the host, one kernel launch per step -, once, on the
  first `--host-rows` rows of the grid (all by default; the host path takes minutes for 100 patterns), a resident signal of
  their own; `device_same_ms` is the device path on those same patterns and `speedup` their ratio;
- `bands_ms`: the band detection alone, which both contain;
- `search_ms` / `search_1_ms`: `Context.hough_optimize_pc` alone with the default evaluations per launch and with ONE
  evaluation per lane and launch; `launch_1_ms` = `search_1_ms` / `launches_1` is what one launch of one evaluation per
  lane costs, launch and the download of the done flags included - the upper estimate of one evaluation that the default
  number per launch rests on (`default_launch_ms_estimate` = `evals_per_launch_default` of them).
`same_bits`: whether the two paths returned the same PCs."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t) * 1e3


def best(fn, reps):
    runs = [timed(fn) for _ in range(reps + 1)]  # the first call is the warm-up (code objects, buffers)
    return runs[-1][0], min(ms for _, ms in runs[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-rows", type=int, default=0, help="rows of the grid the host path is timed on (0: all, minutes for "
                    "a 10 x 10 grid; negative: skip the host path)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hough_pc_search.json"))
    args = ap.parse_args()
    import kikuchipy_amd as kpa

    g = np.load(os.path.join(ROOT, "tests", "golden", "projection.npz"))
    master = kpa.EBSDMasterPattern(np.stack([g["mp_upper"], g["mp_lower"]]).astype(np.float32), hemisphere="both")
    n, shape = args.grid, (60, 60)
    rng = np.random.default_rng(0)
    q = rng.standard_normal((n * n, 4))
    q /= np.sqrt(np.sum(q * q, axis=1))[:, None]
    i, j = np.indices((n, n))
    truth = np.stack([0.42 - 0.002 * j, 0.22 + 0.0015 * i, 0.50 - 0.0006 * i], axis=-1)
    data = np.asarray(master.get_patterns(q, kpa.EBSDDetector(shape, pc=truth.reshape(-1, 3)), compute=True).data, dtype=np.float32)
    s = kpa.EBSD(data.reshape((n, n) + shape)).to_device()
    pc0 = truth.reshape(-1, 3).mean(axis=0)
    ix = kpa.EBSDDetector(shape, pc=pc0).get_indexer("m-3m")
    phase = ix.phaselist[0]
    call = (shape, ix.sample_to_detector, phase.normals, phase.family, phase.angles, ix.tolerance(pc0))
    os.environ.pop("KPDI_HOUGH_PC_SEARCH", None)
    os.environ.pop("KPDI_HOUGH_SEARCH_EVALS", None)
    try:
        bands, bands_ms = best(lambda: ix.detect_bands(s._resident.flat(), s.context), args.reps)
        device, device_ms = best(lambda: s.hough_indexing_optimize_pc(pc0, ix, batch=True), args.reps)
        (_, _, nfev, _, _), search_ms = best(lambda: s.context.hough_optimize_pc(bands, pc0, *call), args.reps)
        _, search_1_ms = best(lambda: s.context.hough_optimize_pc(bands, pc0, *call, evals_per_launch=1), 1)
        host_ms = device_same_ms = same = None
        rows = n if args.host_rows == 0 else min(args.host_rows, n)
        if rows > 0:
            part = s if rows == n else kpa.EBSD(data.reshape((n, n) + shape)[:rows].copy()).to_device()
            try:
                device_part, device_same_ms = best(lambda: part.hough_indexing_optimize_pc(pc0, ix, batch=True), args.reps)
                os.environ["KPDI_HOUGH_PC_SEARCH"] = "host"
                host, host_ms = timed(lambda: part.hough_indexing_optimize_pc(pc0, ix, batch=True))
                os.environ.pop("KPDI_HOUGH_PC_SEARCH")
            finally:
                if part is not s:
                    part.close()
            same = bool(np.array_equal(np.ascontiguousarray(host.pc).view(np.uint64), np.ascontiguousarray(device_part.pc).view(np.uint64))
                        and np.array_equal(device_part.pc, device.pc[:rows]))
    finally:
        s.close()
    launches_1 = int(nfev.max())  # one evaluation per lane and launch: as many launches as the longest search has evaluations
    launch_1_ms = search_1_ms / launches_1
    row = dict(case="hough_pc_search", patterns=n * n, shape=list(shape), version=kpa._lib.version(), bands_ms=bands_ms,
               device_ms=device_ms, host_patterns=max(rows, 0) * n, host_ms=host_ms, device_same_ms=device_same_ms,
               speedup=None if host_ms is None else host_ms / device_same_ms, same_bits=same,
               search_ms=search_ms, search_1_ms=search_1_ms, launches_1=launches_1, launch_1_ms=launch_1_ms,
               evals_per_launch_default=kpa._lib.HOUGH_SEARCH_EVALS,
               default_launch_ms_estimate=kpa._lib.HOUGH_SEARCH_EVALS * launch_1_ms, nfev_mean=float(nfev.mean()),
               nfev_max=int(nfev.max()), rms_pc_error=float(np.sqrt(np.mean((device.pc - truth) ** 2))))
    print(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
