"""Hough indexing (csrc/hough.hip) on one GPU: a resident `--map` x `--map` map (256) of 60 x 60 uint8 patterns, seeded
noise over drawn bands.  Prints one JSON line and writes it to `--out` (profiles/hough_bench.json).

Host-clock times, best of `--reps` warm calls, each ending with the stream synchronised by the result download:
- `bands_ms`: `HoughIndexer.detect_bands` - the Radon and the band kernel over the passes, and the download of `band_data`;
- `index_ms`: `HoughIndexer.index_bands` - upload of the bands, the index kernel, download of the results;
- `call_ms`: the whole of `EBSD.hough_indexing`;
- `copy_ms`: a device-to-device copy of the same patterns into a second context (`EBSD.deepcopy`), the yardstick.
The library has no per-kernel event timers for these kernels: the three are not timed apart."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, reps):
    times = []
    for _ in range(reps + 1):  # the first call is the warm-up (code objects, buffers)
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return out, min(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hough_bench.json"))
    args = ap.parse_args()
    import kikuchipy_amd as kpa

    rng = np.random.default_rng(0)
    i, j = np.mgrid[0:60, 0:60]
    base = sum(np.exp(-0.5 * ((np.cos(t) * (j - 29.5) + np.sin(t) * (i - 29.5) - r) / 1.5) ** 2)
               for t, r in ((0.3, 4.0), (1.2, -9.0), (2.0, 12.0), (2.7, -3.0)))
    m = args.map * args.map
    patterns = np.clip(60 * base[None] + rng.integers(0, 60, (m, 60, 60)), 0, 255).astype(np.uint8)
    s = kpa.EBSD(patterns.reshape(args.map, args.map, 60, 60)).to_device()
    det = kpa.EBSDDetector((60, 60), pc=(0.42, 0.22, 0.5))
    ix = det.get_indexer("m-3m")
    try:
        bands, bands_ms = best(lambda: ix.detect_bands(s._resident.flat(), s.context), args.reps)
        _, index_ms = best(lambda: ix.index_bands(bands, ix.PC, s.context), args.reps)
        xmap, call_ms = best(lambda: s.hough_indexing("m-3m", ix, verbose=0), args.reps)

        def copy():
            twin = s.deepcopy()
            twin.context.synchronize()
            twin.close()

        _, copy_ms = best(copy, args.reps)
    finally:
        s.close()
    row = dict(case="hough", patterns=m, shape=[60, 60], version=kpa._lib.version(), bands_ms=bands_ms, index_ms=index_ms,
               call_ms=call_ms, copy_ms=copy_ms, patterns_per_second=m / (call_ms * 1e-3),
               indexed=int((xmap.phase_id >= 0).sum()))
    print(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
