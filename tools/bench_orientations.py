"""The orientation kernels (csrc/orientations.hip) on one GPU; prints one JSON line per case and writes them to `--out`.

- `outer`: `disorientation_angle_outer` at N = M = `--n` (8192) for 432 and for 1, float64 and float32 output.
  `kernel_ms`: the kernel alone between events on the library's stream (`orientation_ms` of the counters with profiling
  on, summed over the row passes), best of `--reps` warm calls; `call_ms`: the whole call on the host clock, download of
  the N x M result included.  `copy_ms` / `fill_ms`: a device-to-device copy / a fill of the same number of output bytes,
  timed between events in the same run (hipMemcpyAsync / hipMemsetAsync): the floor of a store-bound kernel.
  `kernel_over_copy`, `kernel_over_fill`: the yardsticks.
- `outer_vs_host`: the whole call at N = M = `--host-n` (1024), 432, next to the NumPy host path of the same function.
- `pairs`, `kam`: `disorientation_angle` of a `--map` x `--map` map (512) against one reference orientation, and
  `kernel_average_misorientation_map` with the default window, 432: `kernel_ms` and `call_ms`.
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
    return out, min(times[1:])


def device_floor(n_bytes, reps):
    """(copy_ms, fill_ms) of `n_bytes` on the device: hipMemcpyAsync device to device and hipMemsetAsync between two
    events, through the HIP runtime the library itself is linked against."""
    import ctypes as C

    hip = None
    for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    if hip is None:
        raise RuntimeError("the HIP runtime library was not found")

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(n_bytes)))
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(n_bytes)))
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))
    ok(hip.hipMemset(src, 0, C.c_size_t(n_bytes)))
    out = []
    try:
        for op in (lambda: hip.hipMemcpyAsync(dst, src, C.c_size_t(n_bytes), 3, None),  # hipMemcpyDeviceToDevice
                   lambda: hip.hipMemsetAsync(dst, 1, C.c_size_t(n_bytes), None)):
            times = []
            for _ in range(reps + 1):
                ms = C.c_float()
                ok(hip.hipEventRecord(e0, None))
                ok(op())
                ok(hip.hipEventRecord(e1, None))
                ok(hip.hipEventSynchronize(e1))
                ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
                times.append(ms.value)
            out.append(min(times[1:]))
    finally:
        hip.hipEventDestroy(e0)
        hip.hipEventDestroy(e1)
        hip.hipFree(src)
        hip.hipFree(dst)
    return tuple(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--host-n", type=int, default=1024)
    ap.add_argument("--map", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    rng = np.random.default_rng(0)
    q = rng.standard_normal((args.n, 4))
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)

    with _lib.Context(0) as ctx:
        ctx.set_profiling(1)
        floors = {dtype: device_floor(args.n * args.n * np.dtype(dtype).itemsize, args.reps) for dtype in ("float64", "float32")}

        def timed(fn):
            kernel = []

            def call():
                out = fn()
                kernel.append(ctx.counters()["orientation_ms"])
                return out

            out, call_ms = best(call, args.reps)
            return out, min(kernel[1:]), call_ms

        for dtype in ("float64", "float32"):
            n_bytes = args.n * args.n * np.dtype(dtype).itemsize
            copy_ms, fill_ms = floors[dtype]
            for group in ("432", "1"):
                _, kernel_ms, call_ms = timed(lambda: kpa.disorientation_angle_outer(q, None, group, dtype_out=dtype, context=ctx))
                emit({"case": "outer", "n": args.n, "m": args.n, "point_group": group, "dtype_out": dtype, "output_bytes": n_bytes,
                      "kernel_ms": kernel_ms, "call_ms": call_ms, "copy_ms": copy_ms, "fill_ms": fill_ms,
                      "kernel_over_copy": kernel_ms / copy_ms, "kernel_over_fill": kernel_ms / fill_ms,
                      "pairs_per_second": args.n * args.n / (kernel_ms * 1e-3)})
        h = q[:args.host_n]
        dev, _, call_ms = timed(lambda: kpa.disorientation_angle_outer(h, None, "432", context=ctx))
        t = time.perf_counter()
        host = kpa.disorientation_angle_outer(h, None, "432")
        host_ms = (time.perf_counter() - t) * 1e3
        emit({"case": "outer_vs_host", "n": args.host_n, "m": args.host_n, "point_group": "432", "device_call_ms": call_ms,
              "numpy_host_ms": host_ms, "host_over_device": host_ms / call_ms, "max_abs_difference": float(np.abs(dev - host).max())})
        grid = rng.standard_normal((args.map, args.map, 4))
        _, kernel_ms, call_ms = timed(lambda: kpa.disorientation_angle(grid, q[0], "432", context=ctx))
        emit({"case": "pairs", "map": [args.map, args.map], "point_group": "432", "kernel_ms": kernel_ms, "call_ms": call_ms})
        _, kernel_ms, call_ms = timed(lambda: kpa.kernel_average_misorientation_map(grid, "432", context=ctx))
        emit({"case": "kam", "map": [args.map, args.map], "point_group": "432", "window": "circular (3, 3)", "kernel_ms": kernel_ms,
              "call_ms": call_ms})
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/bench_orientations.py", "library": _lib.version(), "reps": args.reps, "cases": lines}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
