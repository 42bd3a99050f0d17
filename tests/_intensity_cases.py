"""Cases of the intensity fixture (tests/golden/intensity.npz, made by tools/gen_intensity_golden.py): the keyword
arguments of `EBSD.rescale_intensity` / `EBSD.normalize_intensity` each case runs, the inputs beyond the existing
fixtures, and the dtypes."""

import numpy as np

DTYPES = ["uint8", "int8", "uint16", "int16", "float32", "float64"]

RESCALE = {
    "default": {},
    "relative": {"relative": True},
    "in_range": {"in_range": (50, 200)},
    "in_range_wide": {"in_range": (-10, 300)},  # bounds outside uint8 / int8
    "in_range_float": {"in_range": (10.5, 200.25)},
    "out_range": {"out_range": (10, 245)},
    "percentiles": {"percentiles": (0.5, 99.5)},
    "percentiles_1_99": {"percentiles": (1, 99)},
    "percentiles_f32": {"percentiles": (0.5, 99.5), "dtype_out": "float32"},
    "relative_out_range": {"relative": True, "out_range": (10, 245)},
}
RESCALE.update({f"dtype_{d}": {"dtype_out": d} for d in DTYPES})

NORMALIZE = {
    "default": {},
    "sqrt": {"divide_by_square_root": True, "dtype_out": "float32"},
    "std2": {"num_std": 2, "dtype_out": "float32"},
}
NORMALIZE.update({f"dtype_{d}": {"dtype_out": d} for d in DTYPES})

# every case on the Ni patterns and the 3 x 3 dummy; on the synthetic stacks and the degenerate stacks these
SYNTHETIC_RESCALE = ["default", "relative", "in_range", "percentiles", "percentiles_1_99", "dtype_float32", "dtype_uint8",
                     "dtype_int16"]
SYNTHETIC_NORMALIZE = ["default", "dtype_float32", "dtype_float64", "sqrt"]
MAX_STORED_PIXELS = 128 * 96


def as_dtype(stack, dtype):
    """The same pattern values in another dtype: integer patterns shifted into a signed type's range, float patterns
    cast; float patterns to integers are rounded."""
    stack = np.asarray(stack)
    dt = np.dtype(dtype)
    v = stack.astype(np.float64)
    if stack.dtype.kind == "u" and dt.kind == "i":
        v = v - (np.iinfo(stack.dtype).max + 1) // 2
    if dt.kind in "iu":
        info = np.iinfo(dt)
        v = np.clip(np.round(v), info.min, info.max)
    return v.astype(dt)


def degenerate(dtype):
    """Five 16 x 16 patterns: ordinary, one NaN pixel, one +inf pixel, constant, all NaN (the last three as constant
    patterns of other values for integer dtypes)."""
    y, x = np.mgrid[:16, :16]
    base = ((3 * y + 5 * x) % 23).astype(np.float64) * 7 + 20
    s = np.stack([base, base, base, np.full_like(base, 3.0), np.full_like(base, np.nan)])
    s[1, 4, 5] = np.nan
    s[2, 7, 3] = np.inf
    if np.dtype(dtype).kind in "iu":
        s[1, 4, 5] = 100
        s[2, 7, 3] = 120
        s[4] = 90
    return s.astype(dtype)
