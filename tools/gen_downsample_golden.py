"""Write tests/golden/downsample.npz by RUNNING THE REFERENCE ITSELF: its pattern/_pattern.py `_downsample2d` (the
py_func, Numba being stubbed by oracle/ref_shim.py) the way EBSD.downsample (signals/ebsd.py:1113-1219) maps it, and its
`pattern.get_dynamic_background` set-up with pattern/chunk.py's `get_dynamic_background` loop (loaded unmodified with
`ref_shim._load`) and `_fft_filter` / `scipy.ndimage.gaussian_filter`, the way EBSD.get_dynamic_background
(signals/ebsd.py:698-803) runs them: the patterns are cast to `dtype_out` first.  Test infrastructure; run it where the
reference's sources are:

    /opt/conda/bin/python3.9 -W ignore tools/gen_downsample_golden.py

Only data goes in: the expected patterns, the known answers of the reference's tests/test_pattern/test_pattern.py
(TestGetDynamicBackgroundPattern) and tests/test_pattern/test_chunk.py (TestGetDynamicBackgroundChunk), the distance
between the float64 restatement (tests/_downsample_restate.py) and the reference for every background case
(`bgdist__*`: max |difference| for float results; share of differing values and max difference in levels for integer
ones), and the versions that made them (`made_by`).  Cases and inputs: tests/_downsample_cases.py.
"""

import ast
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _downsample_cases as cases  # noqa: E402
import _downsample_restate as restate  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    import scipy
    from scipy.ndimage import gaussian_filter
    from skimage.util.dtype import dtype_range

    pat = ref_shim.load_reference()["pattern"]
    chunk = ref_shim._load("kikuchipy.pattern.chunk", "pattern/chunk.py")

    def downsample(stack, factor, dtype_out):
        dtype_out = stack.dtype.type if dtype_out is None else np.dtype(dtype_out).type
        omin, omax = dtype_range[dtype_out]
        with np.errstate(all="ignore"):
            return np.stack([pat._downsample2d(p, factor, omin, omax, dtype_out) for p in stack])

    def background(stack, filter_domain="frequency", std=None, truncate=4.0, dtype_out=None):
        if std is None:
            std = stack.shape[-1] / 8
        kwargs = {}
        if filter_domain == "frequency":
            filter_func = pat._fft_filter
            (kwargs["fft_shape"], kwargs["window_shape"], kwargs["transfer_function"], kwargs["offset_before_fft"],
             kwargs["offset_after_ifft"]) = pat._dynamic_background_frequency_space_setup(
                pattern_shape=stack.shape[-2:], std=std, truncate=truncate)
        else:
            filter_func = gaussian_filter
            kwargs["sigma"] = std
            kwargs["truncate"] = truncate
        dtype_out = stack.dtype if dtype_out is None else np.dtype(dtype_out)
        with np.errstate(all="ignore"):
            return chunk.get_dynamic_background(stack.astype(dtype_out), filter_func=filter_func, dtype_out=dtype_out,
                                                **kwargs)

    out = {"made_by": np.array(f"the reference's _downsample2d / get_dynamic_background under python "
                               f"{platform.python_version()}, numpy {np.__version__}, scipy {scipy.__version__}")}
    inputs = cases.inputs()
    for name, factor, dtype_out in cases.downsample_cases():
        out[cases.key("ds", name, factor, dtype_out)] = downsample(inputs[name][: cases.stored(name)], factor, dtype_out)
    worst_share, worst_levels = 0.0, 0
    for name, case, dtype_out in cases.background_cases():
        stack = inputs[name]
        kw = cases.BACKGROUND[case]
        ref = background(stack, dtype_out=dtype_out, **kw)
        k = cases.key("bg", name, case, dtype_out)
        out[k] = ref[: cases.BG_STORED]
        mine = restate.get_dynamic_background(stack, dtype_out=dtype_out, **kw)
        # the single-pattern function agrees with the loop when the dtype stays
        if dtype_out is None:
            one = pat.get_dynamic_background(stack[0], **kw)
            assert one.dtype == stack.dtype and np.array_equal(one, ref[0], equal_nan=True), k
        if ref.dtype.kind == "f":
            d = float(np.max(np.abs(mine.astype(np.float64) - ref.astype(np.float64))))
            out["bgdist__" + k] = np.array([d, float(np.max(np.abs(ref)))])
        else:
            diff = np.abs(mine.astype(np.int64) - ref.astype(np.int64))
            share, levels = float(np.mean(diff != 0)), int(diff.max())
            out["bgdist__" + k] = np.array([share, levels])
            worst_share, worst_levels = max(worst_share, share), max(worst_levels, levels)
        print(k, out["bgdist__" + k], flush=True)
    print("integer cases: worst share", worst_share, "worst difference", worst_levels, "levels")
    known(out)
    path = os.path.join(GOLDEN, "downsample.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


def known(out):
    """The parametrized answers of the reference's dynamic-background tests (the dummy signal's pattern (0, 0))."""
    for rel, cls in (("test_pattern/test_pattern.py", "TestGetDynamicBackgroundPattern"),
                     ("test_pattern/test_chunk.py", "TestGetDynamicBackgroundChunk")):
        path = os.path.join(ref_shim.REF_ROOT, "tests", rel)
        tree = ast.parse(open(path).read())
        klass = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0]
        for node in klass.body:
            if not isinstance(node, ast.FunctionDef):
                continue
            for deco in node.decorator_list:
                if isinstance(deco, ast.Call) and getattr(deco.func, "attr", "") == "parametrize":
                    names = [n.strip() for n in ast.literal_eval(deco.args[0]).split(",")]
                    values = eval(compile(ast.Expression(deco.args[1]), path, "eval"), {"np": np})
                    for i, row in enumerate(values):
                        if len(names) == 1:
                            row = (row,)
                        for n, v in zip(names, row):
                            key = f"known__{cls}__{node.name}__{i}__{n}"
                            out[key] = np.array("None") if v is None else np.asarray(v)


if __name__ == "__main__":
    main()
