"""Adaptive histogram equalization throughput on one GPU; prints one JSON line and writes it to
`<out>/clahe_bench.json`, with the parity check in `<out>/clahe_parity.json` (default out: profiles/).

Workloads: uint8 60 x 60 with M = 262 144 patterns and uint8 240 x 240 with M = 4096, the defaults (kernel sx // 4 x
sy // 4, nbins=128) with clip_limit 0 and 0.01.  For each:
- `resident_call_ms`: kpdi_adaptive_histogram_equalization on patterns already in device memory (best of `--reps`),
  host clock around the call and a device synchronise; the patterns are re-uploaded (not timed) before each rep so
  that every rep equalizes the same input; the kernel time alone comes from `rocprofv3 --kernel-trace --stats` over
  this tool (`profiles/clahe_kernel_stats.csv`);
- `pixels_per_s`: M * sy * sx over resident_call_ms;
- `ebsd_call_ms`: EBSD.adaptive_histogram_equalization(inplace=False) from host memory (upload + compute + download).
Parity: the first 64 patterns of each workload against the NumPy restatement (tests/_clahe_restate.py), and the two
kernel paths (KPDI_CLAHE_PATH=1) against each other.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLIPS = {"clip_0": 0.0, "clip_0.01": 0.01}


def one(sy, sx, m, reps, parity):
    import _clahe_restate as R
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _lib
    from kikuchipy_amd.pattern._pattern import clahe_arguments, clahe_kernel_size

    rng = np.random.default_rng(0)
    y, x = np.mgrid[:sy, :sx]
    ramp = (((3 * y + 5 * x) % 97) * 1.5).astype(np.uint8)
    data = (rng.integers(0, 110, (m, sy, sx), dtype=np.uint8) + ramp).astype(np.uint8)
    kernel = clahe_kernel_size(None, (sy, sx))
    res = {"shape": [sy, sx], "dtype": "uint8", "m": m, "kernel": kernel, "nbins": 128}
    with _lib.Context(0) as ctx:
        ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
        for name, clip in CLIPS.items():
            args = clahe_arguments(data[:1], kernel, clip, 128)
            ctx.set_experimental(data)
            ctx.adaptive_histogram_equalization(*args)  # warm-up (code objects, buffers)
            ctx.synchronize()
            times = []
            for _ in range(reps):
                ctx.set_experimental(data)
                t = time.perf_counter()
                ctx.adaptive_histogram_equalization(*args)
                ctx.synchronize()
                times.append(time.perf_counter() - t)
            best = min(times)
            got = ctx.get_experimental()
            r = {"clip_count": args[2], "resident_call_ms": round(best * 1e3, 3),
                 "resident_call_ms_all": [round(c * 1e3, 3) for c in times],
                 "pixels_per_s": float(f"{m * sy * sx / best:.4g}")}
            s = kpa.EBSD(data, device=0)
            s.adaptive_histogram_equalization(clip_limit=clip, inplace=False)
            ebsd = []
            for _ in range(2):
                t = time.perf_counter()
                s2 = s.adaptive_histogram_equalization(clip_limit=clip, inplace=False)
                ebsd.append(time.perf_counter() - t)
            s.close()
            assert np.array_equal(s2.data, got)
            r["ebsd_call_ms"] = round(min(ebsd) * 1e3, 3)
            res[name] = r
            k = min(64, m)
            want = R.ebsd_equalize(data[:k], None, clip, 128)
            os.environ["KPDI_CLAHE_PATH"] = "1"
            try:
                ctx.set_experimental(data[:k])
                ctx.adaptive_histogram_equalization(*args)
                ws = ctx.get_experimental()
            finally:
                del os.environ["KPDI_CLAHE_PATH"]
            parity[f"{sy}x{sx}__{name}"] = {
                "patterns": k, "lds_path_equals_restatement": bool(np.array_equal(got[:k], want)),
                "workspace_path_equals_lds_path": bool(np.array_equal(ws, got[:k]))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m60", type=int, default=262144)
    ap.add_argument("--m240", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    parity = {}
    out = {"tool": "bench_clahe", "version": _lib.version(),
           "shape_60x60": one(60, 60, args.m60, args.reps, parity),
           "shape_240x240": one(240, 240, args.m240, args.reps, parity)}
    line = json.dumps(out)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "clahe_bench.json"), "w") as f:
        f.write(line + "\n")
    with open(os.path.join(args.out, "clahe_parity.json"), "w") as f:
        json.dump(parity, f, indent=1)
    if not all(v["lds_path_equals_restatement"] and v["workspace_path_equals_lds_path"] for v in parity.values()):
        raise SystemExit(f"parity failed: {parity}")


if __name__ == "__main__":
    main()
