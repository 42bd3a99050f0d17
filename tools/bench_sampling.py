"""`get_sample_fundamental` on the host and on one GPU; prints one JSON line per case and writes them to `--out`.

The cases: `resolution` 3, 2 and 1 degrees (45, 67 and 137 steps per semi-edge: 0.75, 2.5 and 20.8 million grid points)
for `m-3m` and `6/mmm`.
- `host_ms`: the NumPy sampler (no `device`), one run on the host clock; for `m-3m` this is the path the package had
  before the kernel existed;
- `kernel_ms`: the kernels alone (count pass, scan, emit pass), between events on the library's stream (`sampling_ms` of
  the counters with profiling on: the count call's and the fill call's, added), best of `--reps` warm calls;
- `call_ms`: `Context.sample_fundamental` on the host clock, best of `--reps` warm calls: both library calls, the
  readback of 32 bytes per kept orientation (the call ends in a synchronise) and the NumPy array;
- `kept`, `max_abs_difference`: the device result against the host's (same shape; the components differ in their last
  bits: tests/test_gpu_sampling.py holds both to the longdouble restatement).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=float, nargs="+", default=[3, 2, 1])
    ap.add_argument("--point-groups", nargs="+", default=["m-3m", "6/mmm"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host sampler (tens of seconds at 1 degree)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from kikuchipy_amd import _lib, sampling

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    lines = []
    with _lib.Context(0) as ctx:
        ctx.set_profiling(1)
        for name in args.point_groups:
            faces = sampling.fundamental_zone_faces(sampling.rotation_group_name(name))
            for resolution in args.resolutions:
                n = sampling.resolution_to_semi_edge_steps(resolution)
                kernel, call = [], []
                for _ in range(args.reps + 1):  # the first call is the warm-up (code object, buffers)
                    t = time.perf_counter()
                    got = sampling.get_sample_fundamental(resolution, name, context=ctx)
                    call.append((time.perf_counter() - t) * 1e3)
                    fill_ms = ctx.counters()["sampling_ms"]
                    count = _lib.C.c_int64(0)  # the count pass alone, as the call above ran it before its fill
                    _lib.check(ctx._f.sample_fundamental_count(ctx._h, n, _lib._ptr(np.ascontiguousarray(faces)), len(faces),
                                                               _lib.C.byref(count)))
                    kernel.append(fill_ms + ctx.counters()["sampling_ms"])
                res = {"tool": "bench_sampling", "version": _lib.version(), "point_group": name, "resolution": resolution,
                       "semi_edge_steps": n, "grid_points": (2 * n + 1) ** 3, "kept": int(got.shape[0]),
                       "kernel_ms": round(min(kernel[1:]), 4), "kernel_ms_all": [round(k, 4) for k in kernel[1:]],
                       "call_ms": round(min(call[1:]), 3), "call_ms_all": [round(c, 3) for c in call[1:]]}
                if not args.no_host:
                    t = time.perf_counter()
                    want = sampling.get_sample_fundamental(resolution, name)
                    res["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                    assert want.shape == got.shape, (want.shape, got.shape)
                    res["max_abs_difference"] = float(np.abs(want - got).max())
                    res["host_over_call"] = round(res["host_ms"] / res["call_ms"], 1)
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
