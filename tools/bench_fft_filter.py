"""FFT-filter throughput on one GPU; prints one JSON line.

Two workloads: uint8 60 x 60 with M = 262 144 patterns (the LDS path of csrc/fftfilter.hip) and uint8 240 x 240 with
M = 4096 (the workspace path).  Two filters on each:
the tutorial's low x high pass in the frequency domain (`shift=True`) and a 5 x 5 Gaussian kernel in the spatial domain.
For each:
- `resident_call_ms`: kpdi_fft_filter on patterns already in device memory (best of `--reps`; each call filters the
  previous call's result in place), host clock around the call, which ends in a device synchronise and includes the
  upload of the small tables (the kernel time alone comes from `rocprofv3 --kernel-trace --stats` over this tool);
- `pattern_per_s`, and for the frequency domain `f32_peak_fraction`: the DFT cost model (forward and inverse half
  spectrum, 2 x (4 sy (sx/2+1) sx + 8 sy^2 (sx/2+1)) flop per pattern) over resident_call_ms against the 157.3 TFLOP/s
  f32 peak;
- `h2d_ms`: the upload of the same patterns from (pageable) host memory, kpdi_set_experimental, same run;
- `ebsd_call_ms`: the whole `EBSD.fft_filter(..., inplace=False)` from host memory (upload + compute + download);
- `cpu_pattern_per_s`: the same filter with scipy on the host (float32, all host cores) over a sample;
- `dynamic_background_ms` (once per shape): `remove_dynamic_background` (the default Gaussian, frequency domain) on the
  same resident stack, measured as (dynamic + spatial filter) - spatial filter, for comparison with the spatial filter.
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
    return 2 * (4 * sy * h * sx + 8 * sy * sy * h)


def filters(sy, sx):
    import kikuchipy_amd as kpa

    x = np.arange(5) - 2.0
    g = np.exp(-0.5 * x**2)
    return {
        "frequency_lowhigh": ("frequency", True, kpa.filters.lowpass_fft_filter((sy, sx), 22, 10)
                              * kpa.filters.highpass_fft_filter((sy, sx), 1, 0.5)),
        "spatial_gauss5": ("spatial", False, np.outer(g, g) / g.sum() ** 2),
    }


def cpu_rate(stack, domain, shift, tf, workers):
    import scipy.fft
    from scipy.ndimage import correlate

    t = time.perf_counter()
    p = stack.astype(np.float32)
    if domain == "frequency":
        h = np.fft.ifftshift(tf) if shift else tf
        f = np.real(scipy.fft.ifft2(scipy.fft.fft2(p, axes=(1, 2), workers=workers) * h, axes=(1, 2), workers=workers))
    else:
        f = np.stack([correlate(q, tf.astype(np.float32), mode="nearest") for q in p])
    mn, mx = f.min(axis=(1, 2), keepdims=True), f.max(axis=(1, 2), keepdims=True)
    out = ((f - mn) / (mx - mn) * 255).astype(np.uint8)
    dt = time.perf_counter() - t
    assert out.shape == stack.shape
    return len(stack) / dt


def one(sy, sx, m, reps, cpu_sample):
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib
    from kikuchipy_amd.pattern._pattern import fft_filter_table

    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, (m, sy, sx), dtype=np.uint8)
    res = {"shape": [sy, sx], "dtype": "uint8", "m": m, "mb": round(data.nbytes / 2**20, 1)}
    workers = os.cpu_count()
    with _lib.Context(0) as ctx:
        ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
        h2d = []
        for _ in range(2):
            t = time.perf_counter()
            ctx.set_experimental(data)  # synchronises
            h2d.append(time.perf_counter() - t)
        res["h2d_ms"] = round(min(h2d) * 1e3, 3)
        res["h2d_gb_per_s"] = round(data.nbytes / min(h2d) / 1e9, 2)
        for name, (domain, shift, tf) in filters(sy, sx).items():
            code, table = fft_filter_table(tf, domain, shift, (sy, sx))
            ctx.fft_filter(code, table)  # warm-up (code objects, buffers)
            calls = []
            for _ in range(reps):
                t = time.perf_counter()
                ctx.fft_filter(code, table)
                calls.append(time.perf_counter() - t)
            call = min(calls)
            r = {"resident_call_ms": round(call * 1e3, 3), "resident_call_ms_all": [round(c * 1e3, 3) for c in calls],
                 "pattern_per_s": round(m / call)}
            if domain == "frequency":
                r["dft_mflop_per_pattern"] = round(dft_flop(sy, sx) / 1e6, 4)
                r["f32_peak_fraction"] = round(dft_flop(sy, sx) * m / call / F32_PEAK, 4)
            s = kpa.EBSD(data, device=0)
            s2 = s.fft_filter(tf, domain, shift, inplace=False)
            ebsd = []
            for _ in range(2):
                t = time.perf_counter()
                s2 = s.fft_filter(tf, domain, shift, inplace=False)
                ebsd.append(time.perf_counter() - t)
            s.close()
            assert s2.data.shape == data.shape and s2.data.dtype == np.uint8
            r["ebsd_call_ms"] = round(min(ebsd) * 1e3, 3)
            r["cpu_cores"] = workers
            r["cpu_pattern_per_s"] = round(cpu_rate(data[:cpu_sample], domain, shift, tf, workers))
            r["cpu_sample"] = cpu_sample
            res[name] = r
        # the dynamic background removal's kernel on the same stack: it runs when the next step flushes it
        code, table = fft_filter_table(filters(sy, sx)["spatial_gauss5"][2], "spatial", False, (sy, sx))
        both = []
        for _ in range(reps):
            ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
            t = time.perf_counter()
            ctx.fft_filter(code, table)
            both.append(time.perf_counter() - t)
        res["dynamic_background_ms"] = round((min(both) - res["spatial_gauss5"]["resident_call_ms"] / 1e3) * 1e3, 3)
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
    out = {"tool": "bench_fft_filter", "version": _lib.version(),
           "shape_60x60": one(60, 60, args.m60, args.reps, 4096),
           "shape_240x240": one(240, 240, args.m240, args.reps, 256)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
