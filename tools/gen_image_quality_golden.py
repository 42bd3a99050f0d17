"""Write tests/golden/image_quality.npz by RUNNING THE REFERENCE ITSELF (its pattern/_pattern.py get_image_quality,
loaded unmodified through oracle/ref_shim.py).  Test infrastructure; run it where the reference's sources are:

    /opt/conda/bin/python3.9 -W ignore tools/gen_image_quality_golden.py

The fixture was made with Python 3.9 and SciPy 1.7.1 (NumPy 1.26.4); the npz records the versions that made it
(`made_by`).  Only data goes in: expected Q values, the seeds of the synthetic stacks (rebuilt at test time by
tests/_iq_inputs.py, integer arithmetic only) and the custom frequency vectors.  Inputs covered:
- the 9 Ni patterns of preproc.npz, raw and after static + dynamic background removal (`ni__static_then_dynamic`);
- synthetic stacks of every shape in _iq_inputs.SHAPES, in uint8, uint16 and float32;
- the 3 x 3 dummy signal of di_dummy.npz (the reference's own known answers);
- custom `frequency_vectors` and / or `inertia_max` on the raw Ni patterns;
each with normalize=True and False.
"""

import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _iq_inputs  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    import scipy

    pat = ref_shim.load_reference()["pattern"]

    def iq(stack, normalize, fv=None, imax=None):
        flat = stack.reshape((-1,) + stack.shape[-2:])
        q = [pat.get_image_quality(p, normalize=normalize, frequency_vectors=fv, inertia_max=imax) for p in flat]
        return np.asarray(q, np.float64).reshape(stack.shape[:-2])

    out = {"made_by": np.array(f"python {platform.python_version()}, scipy {scipy.__version__}, numpy {np.__version__}")}
    pre = np.load(os.path.join(GOLDEN, "preproc.npz"))
    dummy = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    for norm in (True, False):
        t = int(norm)
        out[f"ni__norm{t}"] = iq(pre["ni"], norm)
        out[f"ni_corrected__norm{t}"] = iq(pre["ni__static_then_dynamic"], norm)
        out[f"dummy__norm{t}"] = iq(dummy, norm)
    for si, shape in enumerate(_iq_inputs.SHAPES):
        for di, dtype in enumerate(_iq_inputs.DTYPES):
            seed = 100 * si + di + 1
            key = f"rand__{shape[0]}x{shape[1]}__{dtype}"
            out[key + "__seed"] = np.array(seed)
            s = _iq_inputs.stack(shape, dtype, seed)
            for norm in (True, False):
                out[f"{key}__norm{int(norm)}"] = iq(s, norm)
            print(key, out[key + "__norm1"], flush=True)
    # custom weights: a pattern-independent table unlike the default (not symmetric, not separable)
    k, l = np.mgrid[:60, :60]
    fv = ((7 * k + 3 * l) % 11 + 1 + 0.25 * k).astype(np.float64)
    out["custom__fv"] = fv
    out["custom__inertia_max"] = np.array(1234.5)
    for norm in (True, False):
        t = int(norm)
        out[f"custom_fv__norm{t}"] = iq(pre["ni"], norm, fv=fv)
        out[f"custom_imax__norm{t}"] = iq(pre["ni"], norm, imax=1234.5)
        out[f"custom_both__norm{t}"] = iq(pre["ni"], norm, fv=fv, imax=1234.5)
    np.savez_compressed(os.path.join(GOLDEN, "image_quality.npz"), **out)
    print("wrote", os.path.join(GOLDEN, "image_quality.npz"), out["made_by"])


if __name__ == "__main__":
    main()
