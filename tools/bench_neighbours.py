"""Neighbour averaging and neighbour dot product throughput on one GPU; prints one JSON line and writes it to
`<out>/neighbours_bench.json` (default out: profiles/).

Workload: a 512 x 512 map of 60 x 60 uint8 patterns (262 144), resident, the default window (circular 3 x 3: the four
nearest neighbours).  Each figure is the median of `--reps` warm calls, host clock around the call (every call ends
with a device synchronise):
- `copy_ms`: a device-to-device copy of the stack - the floor of the averaging, which reads and writes the stack at
  least once; `average_ms` and `average_over_copy`;
- `stats_ms`: kpdi_neighbour_dot_products with a 1 x 1 footprint, i.e. the statistics pass alone (it reads the stack
  once) plus an empty pass - the floor of the dot products; `adp_map_ms`, `matrices_ms`, `both_ms` and their ratios;
- `*_gbps`: the stack's own bytes (once for the dot products, twice for copy and averaging) over the time.
The averaging is re-run on its own output from rep to rep (the time does not depend on the values).
The kernel times alone come from `rocprofv3 --kernel-trace --stats` over this tool (profiles/neighbours_kernel_stats.csv).
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(reps, call, sync):
    call()
    sync()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        sync()
        out.append(time.perf_counter() - t)
    return statistics.median(out) * 1e3, [round(v * 1e3, 3) for v in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--ny", type=int, default=512)
    ap.add_argument("--nx", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    import torch

    from kikuchipy_amd import _lib
    from kikuchipy_amd.filters import Window
    from kikuchipy_amd.pattern import _neighbours as N

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    ny, nx, sy, sx = args.ny, args.nx, 60, 60
    rng = np.random.default_rng(0)
    base = rng.integers(0, 200, (sy, sx), dtype=np.uint8)
    data = (base[None] // 2 + rng.integers(0, 128, (ny * nx, sy, sx), dtype=np.uint8)).astype(np.uint8)
    nbytes = data.nbytes
    w = N.window_on_map(Window(), (ny, nx))
    sums = N.neighbour_window_sums(w, ny, nx)
    res = {"tool": "bench_neighbours", "version": _lib.version(), "map": [ny, nx], "shape": [sy, sx], "dtype": "uint8",
           "window": "circular (3, 3)", "reps": args.reps, "stack_bytes": nbytes}
    a = torch.from_numpy(data.reshape(-1)).to("cuda:0")
    b = torch.empty_like(a)
    res["copy_ms"], res["copy_ms_all"] = timed(args.reps, lambda: b.copy_(a), torch.cuda.synchronize)
    del a, b
    torch.cuda.empty_cache()
    with _lib.Context(0) as ctx:
        ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
        ctx.set_experimental(data)
        fp, one = w != 0, np.ones((1, 1), dtype=bool)
        for name, call in (
                ("stats", lambda: ctx.neighbour_dot_products(ny, nx, one, matrices=False)),
                ("adp_map", lambda: ctx.neighbour_dot_products(ny, nx, fp, matrices=False)),
                ("matrices", lambda: ctx.neighbour_dot_products(ny, nx, fp, average=False)),
                ("both", lambda: ctx.neighbour_dot_products(ny, nx, fp)),
                ("average", lambda: ctx.average_neighbour_patterns(ny, nx, w, sums))):
            res[name + "_ms"], res[name + "_ms_all"] = timed(args.reps, call, ctx.synchronize)
    for name in ("adp_map", "matrices", "both"):
        res[name + "_over_stats"] = round(res[name + "_ms"] / res["stats_ms"], 3)
        res[name + "_gbps"] = round(nbytes / res[name + "_ms"] / 1e6, 1)
    res["stats_gbps"] = round(nbytes / res["stats_ms"] / 1e6, 1)
    res["average_over_copy"] = round(res["average_ms"] / res["copy_ms"], 3)
    res["average_gbps"] = round(2 * nbytes / res["average_ms"] / 1e6, 1)
    res["copy_gbps"] = round(2 * nbytes / res["copy_ms"] / 1e6, 1)
    for k in list(res):
        if k.endswith("_ms"):
            res[k] = round(res[k], 3)
    line = json.dumps(res)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "neighbours_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
