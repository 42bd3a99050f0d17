"""The kinematical master pattern on one GPU; prints one JSON line and writes it to `--out`, the parity record to
`--parity`.

The case: `half_size` 500 (1001 x 1001 pixels), both hemispheres, the fcc Ni list of tests/_kinematical_cases.py taken
to |h|, |k|, |l| <= 9 and d >= 0.35 angstrom (1060 reflectors): 2.1e9 pixel-reflector pairs.
- `kernel_ms`: the kernel alone, between two events on the library's stream (`kinematical_ms` of the counters with
  profiling on), best of `--reps` warm calls; `call_ms`: the whole library call on the host clock (directions and table
  formed on the host, two uploads, the kernel, the readback of 16 MB);
- `flop`: 5 per pair (three products and two sums of the dot product; compares and the rare acos are not counted), and
  `share_of_f64_vector_peak` = flop / kernel time over 78.6 TFLOP/s.  MI355X_MICROARCH gives the float32 vector rate
  (157.3 TFLOP/s, 64 FLOP per clock and SIMD, a fused multiply-add counted as two) and no float64 figure; 78.6 is AMD's
  published float64 vector peak, half of it.  The kernel may not contract, so a product and a sum are two instructions:
  half of that peak is the most it can reach;
- `acos_share`: the share of pairs inside the acos screen (csrc/kinematical_plan.h), counted by the NumPy restatement
  over a sample of `--sample` pixels per hemisphere;
- `numpy_ms`: the NumPy restatement (tests/_kinematical_restate.py) of that sample on `--threads` host threads (a block
  of pixels each), scaled to all pixels;
- parity: the kernel against the restatement on the sampled pixels, bit for bit, with the number of pixels the
  comparison leaves out (tests/test_gpu_kinematical.py states the rule).
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

F64_VECTOR_PEAK_TFLOPS = 78.6
SCREEN = 1e-6  # KIN_SCREEN of csrc/kinematical_plan.h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--half-size", type=int, default=500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16384)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parity", default=None)
    args = ap.parse_args()
    import _kinematical_cases as cases
    import _kinematical_restate as R
    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    hkl, theta, f = cases.ni_reflectors(max_index=9, min_d=0.35)
    u, inten = cases.unit_vectors(hkl), abs(f)
    m, hs = int(hkl.shape[0]), args.half_size
    size = 2 * hs + 1
    pairs = 2 * size * size * m
    with _lib.Context(0) as ctx:
        ctx.set_profiling(1)
        kernel, call = [], []
        for _ in range(args.reps + 1):  # the first call is the warm-up (code object, buffers)
            t = time.perf_counter()
            got = ctx.kinematical_master_pattern(u, theta, inten, hs, "both")
            call.append((time.perf_counter() - t) * 1e3)
            kernel.append(ctx.counters()["kinematical_ms"])
    kernel_ms, call_ms = min(kernel[1:]), min(call[1:])
    # the sample: every stride-th pixel of the grid, both hemispheres
    n = size * size
    pick = np.arange(0, n, max(1, n // args.sample))[: args.sample]
    parity, acos, half, band, numpy_s = {}, 0, 0, 0, 0.0
    for h, pole in enumerate((-1, 1)):
        v = cases.directions(hs, pole)[pick]
        blocks = np.array_split(np.arange(len(pick)), args.threads)

        def block(idx):
            c = {}
            return R.get_pattern(inten, v[idx], u, theta, counts=c, screen=SCREEN), c

        t = time.perf_counter()
        with ThreadPoolExecutor(args.threads) as pool:
            parts = list(pool.map(block, blocks))
        numpy_s += time.perf_counter() - t
        want = np.concatenate([p[0] for p in parts])
        acos += sum(p[1]["acos"] for p in parts)
        half += sum(p[1]["half"] for p in parts)
        band += sum(p[1]["band"] for p in parts)
        out = R.near_threshold(v, u, theta)
        mine = got[h].ravel()[pick]
        parity["upper" if pole == -1 else "lower"] = {
            "pixels_compared": int((~out).sum()), "pixels_left_out": int(out.sum()),
            "differing": int((mine[~out] != want[~out]).sum()), "differing_among_left_out": int((mine[out] != want[out]).sum())}
    sampled_pairs = 2 * len(pick) * m
    flop = 5 * pairs
    res = {"tool": "bench_kinematical", "version": _lib.version(), "half_size": hs, "hemispheres": 2, "reflectors": m,
           "pairs": pairs, "kernel_ms": round(kernel_ms, 4), "kernel_ms_all": [round(k, 4) for k in kernel[1:]],
           "call_ms": round(call_ms, 3), "call_ms_all": [round(c, 3) for c in call[1:]],
           "flop": flop, "tflops": round(flop / kernel_ms / 1e9, 3),
           "f64_vector_peak_tflops": F64_VECTOR_PEAK_TFLOPS,
           "share_of_f64_vector_peak": round(flop / kernel_ms / 1e9 / F64_VECTOR_PEAK_TFLOPS, 4),
           "gpairs_per_s": round(pairs / kernel_ms / 1e6, 2),
           "acos_share": acos / sampled_pairs, "half_share": half / sampled_pairs, "band_share": band / sampled_pairs,
           "sample_pixels_per_hemisphere": int(len(pick)),
           "numpy_ms": round(numpy_s * 1e3 * n / len(pick), 1), "numpy_threads": args.threads}
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    if args.parity:
        with open(args.parity, "w") as fh:
            fh.write(json.dumps({"tool": "bench_kinematical", "half_size": hs, "reflectors": m, "parity": parity}) + "\n")
    print(line)
    print(json.dumps(parity))
    assert all(p["differing"] == 0 for p in parity.values()), parity


if __name__ == "__main__":
    main()
