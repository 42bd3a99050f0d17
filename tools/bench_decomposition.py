"""The PCA decomposition on one GPU: M uint8 patterns of 60 x 60 (default M = 40 000); prints one JSON line and writes
it to `--out`.

- `gram`: kpdi_decomposition_gram with centre "signal" on resident patterns, best of `--reps` warm calls, host clock
  around the call.  The call ends in the readback of side^2 float64 (`readback_mb`) and the host's trace check, which
  are inside the clock; `kernel_ms` is the kernel's own time when `--kernel-ms` hands it over (from
  `rocprofv3 --kernel-trace --stats` over this tool).  `flop_counted` is M K^2, one multiply and one add per product of
  the computed triangle; `call_tflops` is it over the call, `kernel_tflops` over the kernel (when known).
- `apply`: the two kpdi_decomposition_apply forms with c = `--components` (upload of the basis and readback inside).
- `model`: kpdi_decomposition_model with c components into float32 (upload of loadings / factors inside; the patterns are
  uploaded again outside the clock before every repetition, since the model replaces them).
- `eigh_ms`: numpy.linalg.eigh of the side x side Gram matrix on the host.
- `numpy_gram_ms`: the same Gram matrix as float64 NumPy on `--threads` threads (the cast of the patterns to float64 and
  the centring are timed apart, `numpy_prepare_ms`), and the largest difference to the GPU's relative to the largest
  entry.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best(fn, reps, before=None):
    times = []
    out = None
    for _ in range(reps + 1):  # the first call is the warm-up (code objects, buffers)
        if before:
            before()
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return min(times[1:]) * 1e3, [round(v * 1e3, 3) for v in times[1:]], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=40000)
    ap.add_argument("--components", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--kernel-ms", type=float, default=None)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", str(args.threads))
    import numpy as np

    from kikuchipy_amd import _lib

    if _lib.device_count() == 0:
        raise SystemExit("no GPU: this tool measures the device and has no CPU fallback")
    sy = sx = 60
    m, k, c = args.m, sy * sx, args.components
    rng = np.random.default_rng(0)
    data = rng.integers(0, 256, (m, sy, sx), dtype=np.uint8)
    out = {"tool": "bench_decomposition", "version": _lib.version(), "m": m, "shape": [sy, sx], "dtype": "uint8",
           "centre": "signal", "components": c}
    with _lib.Context(0) as ctx:
        def upload():
            ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
            ctx.set_experimental(data)

        upload()
        ms, all_ms, (gram, mean, transposed) = best(lambda: ctx.decomposition_gram(_lib.CENTRE_SIGNAL), args.reps)
        side = gram.shape[0]
        flop = float(m) * k * k if not transposed else float(k) * m * m
        out["gram"] = {"side": side, "transposed": bool(transposed), "call_ms": round(ms, 3), "call_ms_all": all_ms,
                       "readback_mb": round(gram.nbytes / 2 ** 20, 1), "flop_counted": flop,
                       "call_tflops": round(flop / ms / 1e9, 3)}
        if args.kernel_ms:
            out["gram"]["kernel_ms"] = args.kernel_ms
            out["gram"]["kernel_tflops"] = round(flop / args.kernel_ms / 1e9, 3)
        t = time.perf_counter()
        lam, vec = np.linalg.eigh(gram)
        out["eigh_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        top = np.ascontiguousarray(vec[:, ::-1][:, :c])
        ms, all_ms, loadings = best(lambda: ctx.decomposition_apply(top, _lib.CENTRE_SIGNAL, False), args.reps)
        out["apply_xc_basis"] = {"call_ms": round(ms, 3), "call_ms_all": all_ms, "out_shape": list(loadings.shape)}
        basis_m = np.ascontiguousarray(loadings)
        ms, all_ms, back = best(lambda: ctx.decomposition_apply(basis_m, _lib.CENTRE_SIGNAL, True), args.reps)
        out["apply_xct_basis"] = {"call_ms": round(ms, 3), "call_ms_all": all_ms, "out_shape": list(back.shape)}
        lo32, fa32 = loadings.astype(np.float32), top.astype(np.float32)

        def model():
            ctx.decomposition_model(lo32, fa32, mean, _lib.CENTRE_SIGNAL, np.float32)
            ctx.synchronize()

        ms, all_ms, _ = best(model, args.reps, before=upload)
        out["model"] = {"call_ms": round(ms, 3), "call_ms_all": all_ms, "dtype_out": "float32"}
        got = ctx.get_experimental()[:4].reshape(4, k)
        want = (loadings[:4].astype(np.float32).astype(np.float64) @ fa32.astype(np.float64).T + mean[:4, None])
        assert np.all(np.abs(got - want.astype(np.float32)) <= np.spacing(np.abs(want.astype(np.float32))))
    if not args.skip_numpy:
        t = time.perf_counter()
        x = data.reshape(m, k).astype(np.float64)
        x -= x.mean(axis=1, keepdims=True)
        out["numpy_prepare_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        t = time.perf_counter()
        g = x.T @ x if not transposed else x @ x.T
        out["numpy_gram_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        out["numpy_threads"] = args.threads
        out["numpy_gram_tflops"] = round(2 * flop / out["numpy_gram_ms"] / 1e9, 3)  # (BLAS computes both triangles)
        out["gram_max_rel_difference"] = float(np.max(np.abs(g - gram)) / np.max(np.abs(g)))
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
