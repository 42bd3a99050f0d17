"""`EBSD.mean` over the map and over the detector on a resident signal, next to a device-to-device copy of the same
patterns and to what a user had before (download, `np.mean` on the host); prints one JSON line per case and writes them
to `--out`.

The cases: a resident `--map` x `--map` map (256) of `--side` x `--side` patterns (60) in uint8 and float32,
`mean((0, 1))` (the mean pattern: the inner axes survive) and `mean((2, 3))` (the mean-intensity map: contiguous runs).
- `kernel_ms`: the kernels of the reduction alone (partials and combine; the mean of float patterns is one pass),
  between events on the library's stream (`preproc_ms` of the counters with profiling on), best of `--reps` warm calls;
- `call_ms`: `s.mean(axis=...)` on the host clock, best of `--reps` warm calls: the library call, the readback of the
  result (the call ends in a synchronise) and the new signal;
- `copy_kernel_ms`: the selection kernel that `deepcopy()` of the resident signal runs (every pattern, whole, into another
  context on the device), between events, best of `--reps`; `copy_call_ms`: `s.deepcopy()` on the host clock;
- `kernel_over_copy`: the yardstick - a reduction reads every byte once, a copy reads and writes every byte;
- `download_ms`, `host_mean_ms`: the alternative, once: `ResidentPatterns.host()` and `np.mean` of that array on this
  machine's host; `bits_equal_numpy` (uint8) / `max_abs_difference` (float32): the device result against it.
"""

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
    for _ in range(reps + 1):  # the first call is the warm-up (code object, buffers)
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return out, min(times[1:]), times[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=256)
    ap.add_argument("--side", type=int, default=60)
    ap.add_argument("--dtypes", nargs="+", default=["uint8", "float32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    lines = []
    rng = np.random.default_rng(0)
    for name in args.dtypes:
        shape = (args.map, args.map, args.side, args.side)
        data = rng.integers(0, 256, shape, dtype=np.uint8) if name == "uint8" else rng.random(shape, dtype=np.float32)
        s = kpa.EBSD(data).to_device()
        ctx = s.context
        ctx.set_profiling(1)

        def copy_kernel():
            with _lib.Context(0) as dst:
                dst.set_profiling(1)
                ctx.select_patterns(into=dst)
                return dst.counters()["preproc_ms"]

        copy_kernel_ms = min(copy_kernel() for _ in range(args.reps + 1))

        def copy_call():
            s.deepcopy()._discard()

        _, copy_call_ms, _ = best(copy_call, args.reps)
        t = time.perf_counter()
        host = s._resident.host()
        download_ms = (time.perf_counter() - t) * 1e3
        for axis in ((0, 1), (2, 3)):
            kernel = []

            def call():
                ctx.reset_counters()
                out = s.mean(axis=axis)
                kernel.append(ctx.counters()["preproc_ms"])
                return out

            got, call_ms, call_all = best(call, args.reps)
            t = time.perf_counter()
            want = host.mean(axis=axis)
            host_mean_ms = (time.perf_counter() - t) * 1e3
            res = {"tool": "bench_reduce", "version": _lib.version(), "dtype": name, "shape": list(shape), "op": "mean",
                   "axis": list(axis), "bytes": int(data.nbytes),
                   "kernel_ms": round(min(kernel[1:]), 4), "kernel_ms_all": [round(k, 4) for k in kernel[1:]],
                   "call_ms": round(call_ms, 3), "call_ms_all": [round(c, 3) for c in call_all],
                   "copy_kernel_ms": round(copy_kernel_ms, 4), "copy_call_ms": round(copy_call_ms, 3),
                   "kernel_over_copy": round(min(kernel[1:]) / copy_kernel_ms, 3),
                   "read_GBps": round(data.nbytes / min(kernel[1:]) / 1e6, 1),
                   "download_ms": round(download_ms, 1), "host_mean_ms": round(host_mean_ms, 1),
                   "host_over_call": round((download_ms + host_mean_ms) / call_ms, 1)}
            if name == "uint8":
                res["bits_equal_numpy"] = bool(got.data.tobytes() == want.tobytes())
            else:
                res["max_abs_difference"] = float(np.abs(got.data.astype(np.float64) - want).max())
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
        s._discard()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
