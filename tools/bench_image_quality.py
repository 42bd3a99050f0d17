"""Image quality throughput on one GPU; prints one JSON line.

Two workloads: uint8 60 x 60 with M = 262 144 patterns (the LDS path of csrc/iq.hip) and uint8 240 x 240 with
M = 4096 (the workspace path).  For each:
- `resident_call_ms`: kpdi_image_quality on patterns already in device memory (best of `--reps`), host clock around
  the call, which ends in a device synchronise and includes the upload of the small tables and the M x 4-byte readback
  (the kernel time alone comes from `rocprofv3 --kernel-trace --stats` over this tool);
- `pattern_per_s` and `f32_peak_fraction`: M / resident_call_ms, and the DFT cost model
  (4 sy (sx/2+1) sx + 8 sy^2 (sx/2+1) flop per pattern) over resident_call_ms against the 157.3 TFLOP/s f32 peak;
- `h2d_ms`: the upload of the same patterns from (pageable) host memory, kpdi_set_experimental, same run;
- `ebsd_call_ms`: the whole `EBSD.get_image_quality` from host memory (upload + compute + readback);
- `cpu_pattern_per_s`: the reference's arithmetic with `scipy.fft.fft2` (float32, all host cores) over a sample.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_PEAK = 157.3e12


def dft_flop(sy, sx):
    h = sx // 2 + 1
    return 4 * sy * h * sx + 8 * sy * sy * h


def cpu_rate(stack, workers):
    import scipy.fft

    from kikuchipy_amd.pattern import fft_frequency_vectors

    sy, sx = stack.shape[-2:]
    w = fft_frequency_vectors((sy, sx))
    imax = w.sum() / (sy * sx)
    t = time.perf_counter()
    p = stack.astype(np.float32)
    p = (p - p.mean(axis=(1, 2), keepdims=True)) / p.std(axis=(1, 2), keepdims=True)
    s = np.abs(scipy.fft.fft2(p, workers=workers))
    q = 1 - ((s * w).sum(axis=(1, 2)) / s.sum(axis=(1, 2))) / imax
    dt = time.perf_counter() - t
    assert np.all(np.isfinite(q))
    return len(stack) / dt


def one(sy, sx, m, reps, cpu_sample):
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
        q = ctx.image_quality(True)  # warm-up (code objects, buffers)
        calls = []
        for _ in range(reps):
            t = time.perf_counter()
            q = ctx.image_quality(True)
            calls.append(time.perf_counter() - t)
    assert q.shape == (m,) and np.all(np.isfinite(q))
    call = min(calls)
    s = kpa.EBSD(data.reshape(m, sy, sx), device=0)
    s.get_image_quality()
    ebsd = []
    for _ in range(2):
        t = time.perf_counter()
        q2 = s.get_image_quality()
        ebsd.append(time.perf_counter() - t)
    s.close()
    assert np.array_equal(q, q2)
    flop = dft_flop(sy, sx) * m
    workers = os.cpu_count()
    res.update({
        "resident_call_ms": round(call * 1e3, 3),
        "resident_call_ms_all": [round(c * 1e3, 3) for c in calls],
        "pattern_per_s": round(m / call),
        "dft_mflop_per_pattern": round(dft_flop(sy, sx) / 1e6, 4),
        "f32_peak_fraction": round(flop / call / F32_PEAK, 4),
        "h2d_ms": round(min(h2d) * 1e3, 3),
        "h2d_gb_per_s": round(data.nbytes / min(h2d) / 1e9, 2),
        "ebsd_call_ms": round(min(ebsd) * 1e3, 3),
        "cpu_cores": workers,
        "cpu_pattern_per_s": round(cpu_rate(data[:cpu_sample], workers)),
        "cpu_sample": cpu_sample,
    })
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
    out = {"tool": "bench_image_quality", "version": _lib.version(),
           "lds_path_60x60": one(60, 60, args.m60, args.reps, 4096),
           "workspace_path_240x240": one(240, 240, args.m240, args.reps, 512)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
