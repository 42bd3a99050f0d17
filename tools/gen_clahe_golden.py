"""Write tests/golden/clahe.npz by RUNNING THE REFERENCE ITSELF (its pattern/_pattern.py
_adaptive_histogram_equalization, i.e. scikit-image's equalize_adapthist then kikuchipy's rescale_intensity, loaded
unmodified through oracle/ref_shim.py), one call per pattern, with the kernel EBSD.adaptive_histogram_equalization
(signals/_kikuchipy_signal.py:340-470) derives: None -> (signal_shape[0] // 4, signal_shape[1] // 4) with HyperSpy's
signal_shape = (sx, sy), a number -> (k, k).  Test infrastructure; run it where the reference's sources are:

    /opt/conda/bin/python3.9 -W ignore tools/gen_clahe_golden.py

Only data goes in: the expected patterns (the first N_STORED of each input), the seeds of the synthetic stacks
(rebuilt at test time by tests/_iq_inputs.py and tests/_clahe_cases.py), the exception type and message the reference
raises for each error case, whether 20000 bins give another result than 16384, and the versions (`made_by`).
Cases: tests/_clahe_cases.py.
"""

import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _clahe_cases as cases  # noqa: E402
import _iq_inputs  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def ebsd_kernel(kernel_size, sig_shape_rc):
    sy, sx = sig_shape_rc
    if kernel_size is None:
        return [sx // 4, sy // 4]
    if np.isscalar(kernel_size):
        return [int(kernel_size)] * 2
    return [int(k) for k in kernel_size]


def main():
    import skimage

    pat = ref_shim.load_reference()["pattern"]

    def run(stack, name, n_stored):
        kernel, clip, nbins = cases.args(name)
        flat = stack.reshape((-1,) + stack.shape[-2:])[:n_stored]
        k = ebsd_kernel(kernel, flat.shape[-2:])
        return np.stack([pat._adaptive_histogram_equalization(p, k, clip, nbins) for p in flat])

    out = {"made_by": np.array(f"python {platform.python_version()}, numpy {np.__version__}, "
                               f"skimage {skimage.__version__}")}
    pre = np.load(os.path.join(GOLDEN, "preproc.npz"))
    for name in cases.NI_CASES:
        out[f"ni__{name}"] = run(pre["ni"], name, 1)
    for name in cases.SHAPE_CASES[:1]:
        out[f"ni_corrected__{name}"] = run(pre["ni__static_then_dynamic"], name, cases.N_STORED)
    for dtype in cases.DTYPES:
        names = cases.SYNTH_CASES[:2] if np.dtype(dtype).kind == "f" else cases.SYNTH_CASES
        n_stored = 1 if np.dtype(dtype).kind == "f" else cases.N_STORED
        seed = 4000 + cases.DTYPES.index(dtype)
        key = f"rand__60x60__{dtype}"
        out[key + "__seed"] = np.array(seed)
        s = cases.as_dtype(_iq_inputs.stack((60, 60), cases.base_dtype(dtype), seed), dtype)
        for name in names:
            out[f"{key}__{name}"] = run(s, name, n_stored)
        for name in cases.DEGENERATE_CASES:
            out[f"degenerate__{dtype}__{name}"] = run(cases.degenerate(dtype), name, 5)
        print(key, flush=True)
    for shape in ((61, 59), (59, 61)):
        key = f"rand__{shape[0]}x{shape[1]}__uint8"
        seed = 4100 + shape[0]
        out[key + "__seed"] = np.array(seed)
        s = _iq_inputs.stack(shape, "uint8", seed)
        for name in cases.SHAPE_CASES:
            out[f"{key}__{name}"] = run(s, name, cases.N_STORED)
    for name, (dtype, shape, kernel, clip, nbins) in cases.ERRORS.items():
        p = cases.error_input(name)
        try:
            pat._adaptive_histogram_equalization(p, ebsd_kernel(kernel, shape), clip, nbins)
            raise SystemExit(f"{name}: the reference raised nothing")
        except (ValueError, ZeroDivisionError) as e:
            out[f"error__{name}"] = np.array([type(e).__name__, str(e)])
    p = pre["ni"].reshape(-1, 60, 60)[0]
    a = pat._adaptive_histogram_equalization(p, [15, 15], 0.01, 20000)
    b = pat._adaptive_histogram_equalization(p, [15, 15], 0.01, 16384)
    out["nbins_20000_differs_from_16384"] = np.array(not np.array_equal(a, b))
    path = os.path.join(GOLDEN, "clahe.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
