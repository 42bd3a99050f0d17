"""Downsampling and the dynamic background on one GPU; prints one JSON line and writes it to `--out`.

Cases, uint8: 60 x 60 with M = 262 144 at factor 2, 240 x 240 with M = 4096 at factor 4, 480 x 480 with M = 1024 at
factor 8 (-> 60 x 60); `get_dynamic_background` (frequency domain, defaults) on the first two.  For each:
- `resident_call_ms`: the library call on patterns already in device memory, best of `--reps` warm calls, host clock
  around the call.  kpdi_downsample replaces the resident patterns, so every repetition uploads them again outside the
  clock and the clock ends at a device synchronise; kpdi_get_dynamic_background ends in the readback of M sy sx values,
  which is inside its clock (`readback_mb`).  The kernel time alone comes from `rocprofv3 --kernel-trace --stats` over
  this tool;
- `bytes_read`: M sy sx itemsize, one pass, and `call_tb_per_s` = bytes_read / resident_call_ms;
- `numpy_ms`: the NumPy restatement (tests/_downsample_restate.py) over a sample on `--threads` host threads (a block
  of patterns each), scaled to M.
"""

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def numpy_ms(fn, sample, threads, m):
    blocks = np.array_split(sample, threads)
    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(fn, blocks))
    return (time.perf_counter() - t) * 1e3 * m / len(sample)


def one(sy, sx, m, factor, reps, sample, threads, background):
    import _downsample_restate as R
    from kikuchipy_amd import _lib

    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, (m, sy, sx), dtype=np.uint8)
    res = {"shape": [sy, sx], "dtype": "uint8", "m": m, "factor": factor, "bytes_read": int(data.nbytes)}
    k = min(len(data), 32)
    with _lib.Context(0) as ctx:
        calls = []
        for _ in range(reps + 1):  # the first call is the warm-up (code objects, buffers)
            ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
            ctx.set_experimental(data)  # synchronises
            t = time.perf_counter()
            ctx.downsample(factor)
            ctx.synchronize()
            calls.append(time.perf_counter() - t)
        out = ctx.get_experimental()
        assert np.array_equal(out[:k], R.downsample_stack(data[:k], factor))
        call = min(calls[1:])
        res["downsample"] = {"resident_call_ms": round(call * 1e3, 3),
                             "resident_call_ms_all": [round(c * 1e3, 3) for c in calls[1:]],
                             "call_tb_per_s": round(data.nbytes / call / 1e12, 3),
                             "numpy_ms": round(numpy_ms(lambda b: R.downsample_stack(b, factor), data[:sample], threads, m), 1),
                             "numpy_threads": threads, "numpy_sample": sample}
        if background:
            ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
            ctx.set_experimental(data)
            calls = []
            for _ in range(reps + 1):
                t = time.perf_counter()
                bg = ctx.get_dynamic_background(_lib.DOMAIN_FREQUENCY, None, 4.0)
                calls.append(time.perf_counter() - t)
            want = R.get_dynamic_background(data[:k])
            diff = np.abs(bg[:k].astype(int) - want.astype(int))
            assert diff.max() <= 1 and np.mean(diff != 0) <= 1e-3
            call = min(calls[1:])
            bsample = max(threads, sample // 8)
            res["dynamic_background"] = {
                "resident_call_ms": round(call * 1e3, 3), "resident_call_ms_all": [round(c * 1e3, 3) for c in calls[1:]],
                "readback_mb": round(bg.nbytes / 2**20, 1),
                "numpy_ms": round(numpy_ms(R.get_dynamic_background, data[:bsample], threads, m), 1),
                "numpy_threads": threads, "numpy_sample": bsample}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m60", type=int, default=262144)
    ap.add_argument("--m240", type=int, default=4096)
    ap.add_argument("--m480", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    out = {"tool": "bench_downsample", "version": _lib.version(),
           "60x60_by_2": one(60, 60, args.m60, 2, args.reps, 16384, args.threads, True),
           "240x240_by_4": one(240, 240, args.m240, 4, args.reps, 512, args.threads, True),
           "480x480_by_8": one(480, 480, args.m480, 8, args.reps, 128, args.threads, False)}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
