"""Virtual BSE region sums on one GPU; prints one JSON line and writes it to `--out`.

Two workloads, uint8: 60 x 60 with M = 262 144 patterns (one block per pattern, csrc/regionsum_plan.h) and 240 x 240 with
M = 4096 (8 blocks per pattern + the final sums), each with the 25 rectangles of a 5 x 5 grid and with the three
rectangles of an RGB image.  For each:
- `resident_call_ms`: kpdi_region_sums on patterns already in device memory (best of `--reps`), host clock around the
  call, which ends in a device synchronise and includes the upload of the rectangles and the readback of M x n_rects
  uint64 (the kernel time alone comes from `rocprofv3 --kernel-trace --stats` over this tool);
- `bytes_read`: M sy sx itemsize, one pass, and `call_tb_per_s` = bytes_read / resident_call_ms;
- `h2d_ms`: the upload of the same patterns from (pageable) host memory, kpdi_set_experimental, same run;
- `numpy_ms`: the reference's slice-and-nansum per rectangle in NumPy over a sample, on `--threads` host threads (a block
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


def grid_rects(sy, sx, gy=5, gx=5):
    rows, cols = np.linspace(0, sy, gy + 1), np.linspace(0, sx, gx + 1)
    return [(int(round(rows[r])), int(round(rows[r] + rows[1])), int(round(cols[c])), int(round(cols[c] + cols[1])))
            for r in range(gy) for c in range(gx)]


def numpy_ms(sample, rects, threads, m):
    blocks = np.array_split(sample, threads)

    def one(block):
        return [np.nansum(block[:, r0:r1, c0:c1], axis=(-2, -1)) for r0, r1, c0, c1 in rects]

    t = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, blocks))
    return (time.perf_counter() - t) * 1e3 * m / len(sample)


def one(sy, sx, m, reps, sample, threads):
    from kikuchipy_amd import _lib

    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, (m, sy, sx), dtype=np.uint8)
    res = {"shape": [sy, sx], "dtype": "uint8", "m": m, "bytes_read": int(data.nbytes)}
    grid = grid_rects(sy, sx)
    with _lib.Context(0) as ctx:
        ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
        h2d = []
        for _ in range(2):
            t = time.perf_counter()
            ctx.set_experimental(data)  # synchronises
            h2d.append(time.perf_counter() - t)
        res["h2d_ms"] = round(min(h2d) * 1e3, 3)
        for name, rects in (("grid_5x5", grid), ("rgb_3", grid[:3])):
            out = ctx.region_sums(rects)  # warm-up (code objects, buffers)
            calls = []
            for _ in range(reps):
                t = time.perf_counter()
                out = ctx.region_sums(rects)
                calls.append(time.perf_counter() - t)
            k = min(len(data), 64)
            want = np.stack([data[:k, r0:r1, c0:c1].sum(axis=(1, 2), dtype=np.uint64) for r0, r1, c0, c1 in rects], axis=-1)
            assert np.array_equal(out[:k], want)
            call = min(calls)
            res[name] = {"n_rects": len(rects), "resident_call_ms": round(call * 1e3, 3),
                         "resident_call_ms_all": [round(c * 1e3, 3) for c in calls],
                         "call_tb_per_s": round(data.nbytes / call / 1e12, 3),
                         "readback_mb": round(out.nbytes / 2**20, 1),
                         "numpy_ms": round(numpy_ms(data[:sample], rects, threads, m), 1), "numpy_threads": threads,
                         "numpy_sample": sample}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m60", type=int, default=262144)
    ap.add_argument("--m240", type=int, default=4096)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    out = {"tool": "bench_vbse", "version": _lib.version(),
           "one_block_60x60": one(60, 60, args.m60, args.reps, 16384, args.threads),
           "blocks_240x240": one(240, 240, args.m240, args.reps, 1024, args.threads)}
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
