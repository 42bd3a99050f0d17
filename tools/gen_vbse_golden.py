"""Write tests/golden/vbse.npz by RUNNING THE REFERENCE ITSELF: its imaging/vbse.py `_normalize_image` and
`_get_rgb_image` and its pattern/_pattern.py `rescale_intensity`, loaded unmodified through oracle/ref_shim.py.  Test
infrastructure; run it where the reference's sources are:

    /opt/conda/bin/python3.9 -W ignore tools/gen_vbse_golden.py

Only data goes in: expected arrays, the numbers of the reference's own tests (`known__*`) and `made_by`; the inputs are
golden arrays and synthetic maps rebuilt at test time (tests/_vbse_cases.py).  The few lines of `VirtualBSEImager` and
`EBSD.get_virtual_bse_intensity` that need HyperSpy are written out here: the ROI as a NumPy slice
(tests/_vbse_restate.py `roi_rect`: HyperSpy's value -> index rule, restated from memory), `nansum` over the two signal
axes as `np.nansum(..., axis=(-2, -1))`, and the loops of `get_images_from_grid` / `get_rgb_image` over tiles and
channels.  Every RGB case is asserted to come out of the restatement's `rgb` with the same bytes.
"""

import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _vbse_cases as cases  # noqa: E402
import _vbse_restate as R  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def main():
    ref = ref_shim.load_reference()
    normalize_image = ref_shim.load_function_source("imaging/vbse.py", "_normalize_image")
    get_rgb_image = ref_shim.load_function_source(
        "imaging/vbse.py", "_get_rgb_image",
        {"_normalize_image": normalize_image, "rescale_intensity": ref["pattern"].rescale_intensity})
    out = {"made_by": np.array(f"python {platform.python_version()}, numpy {np.__version__}")}

    # ---- get_images_from_grid (vbse.py:269-276)
    for inp, grid, dtype_out in cases.GRID_CASES:
        data = cases.inputs(inp)
        key = cases.grid_key(inp, grid, dtype_out)
        out[key] = R.images_from_grid(data, grid, dtype_out)
        print(key, out[key].shape, out[key].dtype, flush=True)
    one = out[cases.grid_key("dummy", (1, 1), "float32")]
    assert np.allclose(one.mean(), cases.KNOWN_DUMMY_1X1_MEAN)
    out["known__dummy_1x1_mean"] = np.array(cases.KNOWN_DUMMY_1X1_MEAN)

    # ---- get_rgb_image (vbse.py:197-227)
    for name, (inp, grid, r, g, b, kw) in cases.RGB_CASES.items():
        data = cases.inputs(inp)
        kw = dict(kw)
        kw["alpha"] = cases.alpha(kw.get("alpha"))
        kw.setdefault("dtype_out", "uint8")
        chans = R.channels(data, grid, r, g, b)
        got = get_rgb_image(channels=[c.copy() for c in chans], **{**kw, "dtype_out": np.dtype(kw["dtype_out"])})
        got = got.astype(np.dtype(kw["dtype_out"]))  # vbse.py:227
        assert got.shape == data.shape[:2] + (3,) and got.dtype == np.dtype(kw["dtype_out"])
        assert np.array_equal(got, R.rgb(chans, **kw)), f"{name}: the restatement is not the reference"
        out[cases.rgb_key(name)] = got
        if name in cases.KNOWN_RGB_MEAN:
            want, atol = cases.KNOWN_RGB_MEAN[name]
            assert cases.close_to_known(got.mean(), want, atol), (name, got.mean(), want)
            out["known__" + name] = np.array(want)
        print(name, got.dtype, round(float(got.mean()), 5), flush=True)
    path = os.path.join(GOLDEN, "vbse.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
