"""Write tests/golden/intensity.npz by RUNNING THE REFERENCE ITSELF (its pattern/_pattern.py rescale_intensity and
normalize_intensity, loaded unmodified through oracle/ref_shim.py), the way EBSD.rescale_intensity /
normalize_intensity (signals/_kikuchipy_signal.py:88-338) map them: `relative` takes the global (data.min(),
data.max()), `dtype_out` defaults to the data's dtype and `out_range` to skimage's dtype_range[dtype_out], then one
call per pattern.  Test infrastructure; run it where the reference's sources are:

    /opt/conda/bin/python3.9 -W ignore tools/gen_intensity_golden.py

Only data goes in: the expected patterns (of the first N stored patterns of each input; `relative` still reduces over
all of them), the seeds of the synthetic stacks (rebuilt at test time by tests/_iq_inputs.py and
tests/_intensity_cases.py), the known answers of the reference's tests/test_signals/test_ebsd.py and of the EBSD
docstring, and the versions that made them (`made_by`).  Cases: tests/_intensity_cases.py.
"""

import ast
import os
import platform
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _intensity_cases as cases  # noqa: E402
import _iq_inputs  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SYNTH_SHAPES = [(61, 59), (60, 60), (1, 64), (64, 1)]


def main():
    import skimage
    from skimage.util.dtype import dtype_range

    pat = ref_shim.load_reference()["pattern"]

    def rescale(stack, relative=False, in_range=None, out_range=None, dtype_out=None, percentiles=None):
        if relative:
            in_range = (stack.min(), stack.max())
        dtype_out = stack.dtype if dtype_out is None else np.dtype(dtype_out)
        if out_range is None:
            out_range = dtype_range[dtype_out.type]
        out = np.empty(stack.shape, dtype=dtype_out)
        for idx in np.ndindex(stack.shape[:-2]):
            out[idx] = pat.rescale_intensity(stack[idx], in_range=in_range, out_range=out_range, dtype_out=dtype_out,
                                             percentiles=percentiles)
        return out

    def normalize(stack, num_std=1, divide_by_square_root=False, dtype_out=None):
        dtype_out = stack.dtype if dtype_out is None else np.dtype(dtype_out)
        out = np.empty(stack.shape, dtype=dtype_out)
        for idx in np.ndindex(stack.shape[:-2]):
            out[idx] = pat.normalize_intensity(stack[idx], num_std, divide_by_square_root, dtype_out)
        return out

    out = {"made_by": np.array(f"python {platform.python_version()}, numpy {np.__version__}, "
                               f"skimage {skimage.__version__}")}

    def run(key, stack, rescale_names, normalize_names, n_stored):
        flat = stack.reshape((-1,) + stack.shape[-2:])
        for name in rescale_names:
            out[f"{key}__rescale__{name}"] = rescale(flat, **cases.RESCALE[name])[:n_stored]
        for name in normalize_names:
            out[f"{key}__normalize__{name}"] = normalize(flat, **cases.NORMALIZE[name])[:n_stored]

    pre = np.load(os.path.join(GOLDEN, "preproc.npz"))
    dummy = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    run("ni", pre["ni"], list(cases.RESCALE), list(cases.NORMALIZE), 1)
    run("ni_corrected", pre["ni__static_then_dynamic"], cases.SYNTHETIC_RESCALE, cases.SYNTHETIC_NORMALIZE, 1)
    for dtype in cases.DTYPES:
        run(f"dummy__{dtype}", cases.as_dtype(dummy, dtype), list(cases.RESCALE), list(cases.NORMALIZE), 9)
        run(f"degenerate__{dtype}", cases.degenerate(dtype), cases.SYNTHETIC_RESCALE, cases.SYNTHETIC_NORMALIZE, 5)
    for si, shape in enumerate(_iq_inputs.SHAPES):
        if tuple(shape) not in SYNTH_SHAPES:
            continue
        for di, base in enumerate(_iq_inputs.DTYPES):
            seed = 3000 + 100 * si + di
            s = _iq_inputs.stack(shape, base, seed)
            # 61 x 59 in every dtype (the signed / float64 ones derived from the base dtypes); the others in the base
            targets = {"uint8": ["uint8", "int8"], "uint16": ["uint16", "int16"], "float32": ["float32", "float64"]}[base]
            if tuple(shape) != (61, 59):
                targets = targets[:1]
            for dtype in targets:
                key = f"rand__{shape[0]}x{shape[1]}__{dtype}"
                out[key + "__seed"] = np.array(seed)
                out[key + "__base"] = np.array(base)
                names_r = ["default", "relative", "percentiles"] if tuple(shape) == (61, 59) else ["default", "percentiles"]
                run(key, cases.as_dtype(s, dtype), names_r, ["dtype_float32"], 1)
                print(key, flush=True)
    known(out)
    path = os.path.join(GOLDEN, "intensity.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


def known(out):
    """The parametrized answers of the reference's test_rescale_intensity, test_rescale_intensity_percentiles and
    test_normalize_intensity (the dummy signal's pattern (0, 0)), and the docstring's relative=True answer for the Ni
    pattern (0, 0)."""
    path = os.path.join(ref_shim.REF_ROOT, "tests", "test_signals", "test_ebsd.py")
    tree = ast.parse(open(path).read())
    for node in ast.walk(tree):
        if not isinstance(node, ast.FunctionDef):
            continue
        if node.name not in ("test_rescale_intensity", "test_rescale_intensity_percentiles", "test_normalize_intensity"):
            continue
        for deco in node.decorator_list:
            if isinstance(deco, ast.Call) and getattr(deco.func, "attr", "") == "parametrize":
                names = [n.strip() for n in ast.literal_eval(deco.args[0]).split(",")]
                values = eval(compile(ast.Expression(deco.args[1]), path, "eval"), {"np": np})
                for i, row in enumerate(values):
                    for n, v in zip(names, row):
                        key = f"known__{node.name}__{i}__{n}"
                        if v is None:
                            out[key] = np.array("None")
                        elif isinstance(v, type):
                            out[key] = np.array(np.dtype(v).name)
                        else:
                            out[key] = np.asarray(v)
    src = open(os.path.join(ref_shim.SRC, "signals", "_kikuchipy_signal.py")).read()
    m = re.search(r"s2\.rescale_intensity\(relative=True\).*?\n\s*uint8 (\d+) (\d+) (\d+) (\d+)", src, re.S)
    out["known__docstring_relative__ni_minmax"] = np.array([int(g) for g in m.groups()])


if __name__ == "__main__":
    main()
