"""Write tests/golden/fft_filter.npz by RUNNING THE REFERENCE ITSELF (its pattern/_pattern.py fft_filter and
rescale_intensity, filters/fft_barnes.py _fft_filter_setup / _fft_filter and filters/window.py, loaded unmodified
through oracle/ref_shim.py), the way EBSD.fft_filter -> pattern/chunk.py fft_filter runs them: every pattern as
float32, filtered, then rescale_intensity(filtered, dtype_out=<input dtype>).  Test infrastructure; run it where the
reference's sources are:

    /opt/conda/bin/python3.9 -W ignore tools/gen_fft_filter_golden.py

Only data goes in: the expected filtered patterns, the seeds of the synthetic stacks (rebuilt at test time by
tests/_iq_inputs.py) and the versions that made them (`made_by`).  Inputs (cases: tests/_fft_filter_cases.py):
- the 9 Ni patterns of preproc.npz, raw with every case and `ni__static_then_dynamic` with NI_CORRECTED_CASES;
- the 3 x 3 dummy of di_dummy.npz as uint8, uint16 and float32 with every case;
- the synthetic stacks of _iq_inputs.SHAPES up to 128 x 96, in uint8, uint16 and float32, one case each
  (synthetic_case), their first N_STORED patterns.
"""

import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _fft_filter_cases as cases  # noqa: E402
import _iq_inputs  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_STORED_PIXELS = 128 * 96


class RefFunctions:
    def __init__(self, ref):
        w = ref["window"]
        self.lowpass = w.lowpass_fft_filter
        self.highpass = w.highpass_fft_filter
        self.hann = w.modified_hann
        self.window = lambda name, shape, **kw: w.Window(name, shape=shape, **kw)


def main():
    import scipy

    ref = ref_shim.load_reference()
    pat, fb = ref["pattern"], ref["fft_barnes"]
    f = RefFunctions(ref)

    def run(stack, name):
        domain, shift, build = cases.CASES[name]
        sig = stack.shape[-2:]
        tf = build(sig, f)
        kw = {}
        if domain == "spatial":
            fft_shape, tf_pad, before, after = fb._fft_filter_setup(sig, tf)
            kw = dict(fft_shape=fft_shape, window_shape=tf.shape, offset_before_fft=before, offset_after_ifft=after)
        out = np.empty_like(stack)
        for idx in np.ndindex(stack.shape[:-2]):
            p = stack[idx].astype(np.float32)
            if domain == "frequency":
                filtered = pat.fft_filter(p, transfer_function=tf, shift=shift)
            else:
                filtered = fb._fft_filter(p, transfer_function=tf_pad, **kw)
            out[idx] = pat.rescale_intensity(filtered, dtype_out=stack.dtype.type)
        return out

    out = {"made_by": np.array(f"python {platform.python_version()}, scipy {scipy.__version__}, numpy {np.__version__}")}
    pre = np.load(os.path.join(GOLDEN, "preproc.npz"))
    dummy = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    for name in cases.NAMES:
        out[f"ni__{name}"] = run(pre["ni"], name)
        for dtype in _iq_inputs.DTYPES:
            out[f"dummy__{dtype}__{name}"] = run(dummy.astype(dtype), name)
    for name in cases.NI_CORRECTED_CASES:
        out[f"ni_corrected__{name}"] = run(pre["ni__static_then_dynamic"], name)
    for si, shape in enumerate(_iq_inputs.SHAPES):
        if shape[0] * shape[1] > MAX_STORED_PIXELS:
            continue
        for di, dtype in enumerate(_iq_inputs.DTYPES):
            seed = 1000 + 100 * si + di
            name = cases.synthetic_case(si, di)
            key = f"rand__{shape[0]}x{shape[1]}__{dtype}"
            s = _iq_inputs.stack(shape, dtype, seed)[: cases.N_STORED]
            out[key + "__seed"] = np.array(seed)
            out[key + "__case"] = np.array(name)
            out[key] = run(s, name)
            print(key, name, flush=True)
    path = os.path.join(GOLDEN, "fft_filter.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
