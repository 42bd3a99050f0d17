"""Intensity rescaling / normalization throughput on one GPU; prints one JSON line.

Two workloads: uint8 60 x 60 with M = 262 144 patterns and uint8 240 x 240 with M = 4096 (both the LDS path of
csrc/intensity.hip).  Four calls on each: the default rescale (in place, uint8 -> uint8), rescale with
dtype_out=float32, rescale with percentiles=(1, 99), normalize with dtype_out=float32.  For each:
- `resident_call_ms`: the kpdi_* call on patterns already in device memory (best of `--reps`), host clock around the
  call, which ends in a device synchronise; calls that change the dtype get a fresh upload (not timed) before each rep;
  the kernel time alone comes from `rocprofv3 --kernel-trace --stats` over this tool;
- `effective_gb_per_s` and `copy_fraction`: bytes read + bytes written over resident_call_ms, against the 6.29 TB/s
  device-to-device copy rate measured on the MI355X;
- `ebsd_call_ms`: the whole EBSD method with inplace=False from host memory (upload + compute + download).
`h2d_ms`: the upload of the same patterns from (pageable) host memory, kpdi_set_experimental.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12

CALLS = {
    "rescale_default": ("rescale", {}, np.uint8),
    "rescale_float32": ("rescale", {"dtype_out": np.float32}, np.float32),
    "rescale_percentiles_1_99": ("rescale", {"percentiles": (1, 99)}, np.uint8),
    "normalize_float32": ("normalize", {"dtype_out": np.float32}, np.float32),
}


def one(sy, sx, m, reps):
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib

    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, (m, sy, sx), dtype=np.uint8)
    res = {"shape": [sy, sx], "dtype": "uint8", "m": m, "mb": round(data.nbytes / 2**20, 1)}
    with _lib.Context(0) as ctx:
        ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
        h2d = []
        for _ in range(2):
            t = time.perf_counter()
            ctx.set_experimental(data)  # synchronises
            h2d.append(time.perf_counter() - t)
        res["h2d_ms"] = round(min(h2d) * 1e3, 3)
        res["h2d_gb_per_s"] = round(data.nbytes / min(h2d) / 1e9, 2)
        for name, (kind, kw, out_dtype) in CALLS.items():
            def call():
                if kind == "rescale":
                    ctx.rescale_intensity(None, kw.get("percentiles"), 0.0,
                                          1.0 if out_dtype == np.float32 else 255.0, kw.get("dtype_out"))
                else:
                    ctx.normalize_intensity(1, False, kw.get("dtype_out"))
                ctx.synchronize()

            fresh = out_dtype != np.uint8
            ctx.set_experimental(data)
            call()  # warm-up (code objects, buffers)
            times = []
            for _ in range(reps):
                if fresh:
                    ctx.set_experimental(data)
                t = time.perf_counter()
                call()
                times.append(time.perf_counter() - t)
            best = min(times)
            moved = data.nbytes * (1 + np.dtype(out_dtype).itemsize)
            r = {"resident_call_ms": round(best * 1e3, 3), "resident_call_ms_all": [round(c * 1e3, 3) for c in times],
                 "effective_gb_per_s": round(moved / best / 1e9, 1),
                 "copy_fraction": round(moved / best / COPY_RATE, 3)}
            s = kpa.EBSD(data, device=0)
            method = s.rescale_intensity if kind == "rescale" else s.normalize_intensity
            method(inplace=False, **kw)
            ebsd = []
            for _ in range(2):
                t = time.perf_counter()
                s2 = method(inplace=False, **kw)
                ebsd.append(time.perf_counter() - t)
            s.close()
            assert s2.data.shape == data.shape and s2.data.dtype == out_dtype
            r["ebsd_call_ms"] = round(min(ebsd) * 1e3, 3)
            res[name] = r
        ctx.set_experimental(data)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m60", type=int, default=262144)
    ap.add_argument("--m240", type=int, default=4096)
    args = ap.parse_args()
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    out = {"tool": "bench_intensity", "version": _lib.version(), "copy_rate_tb_per_s": COPY_RATE / 1e12,
           "shape_60x60": one(60, 60, args.m60, args.reps),
           "shape_240x240": one(240, 240, args.m240, args.reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
