"""Cases of the adaptive histogram equalization fixture (tests/golden/clahe.npz, made by tools/gen_clahe_golden.py):
the (kernel_size, clip_limit, nbins) each case runs, the inputs beyond the existing fixtures, and the dtypes.  Keys:
`<input>__<case>`; a kernel_size of None is the EBSD method's default, (sx // 4, sy // 4) as (rows, cols)."""

import numpy as np

DTYPES = ["uint8", "int8", "uint16", "int16", "float32", "float64"]
KERNELS = {"none": None, "k10": 10, "k7x13": (7, 13), "k1": (1, 1), "k80": (80, 80)}
CLIPS = {"c0": 0, "c001": 0.01, "c005": 0.05, "c1": 1.0}
NBINS = {"b1": 1, "b64": 64, "b128": 128, "b256": 256, "b16384": 16384}


def case(kernel, clip, nbins):
    return f"{kernel}_{clip}_{nbins}"


def args(name):
    """(kernel_size, clip_limit, nbins) of a case name."""
    k, c, b = name.split("_")
    return KERNELS[k], CLIPS[c], NBINS[b]


# the Ni patterns: every clip limit and bin count for the default and the 7 x 13 kernel, fewer for the others
NI_CASES = [case(k, c, b) for k in KERNELS for c in CLIPS for b in NBINS
            if k in ("none", "k7x13") or (c in ("c0", "c001") and b in ("b64", "b128", "b16384"))]
# the synthetic stacks in every dtype (floats: the first two)
SYNTH_CASES = [case("none", "c0", "b128"), case("k7x13", "c001", "b64"), case("none", "c005", "b256"),
               case("k1", "c0", "b128")]
SHAPE_CASES = [case("none", "c0", "b128"), case("none", "c001", "b128")]  # 61 x 59 and 59 x 61
DEGENERATE_CASES = [case("none", "c0", "b128"), case("none", "c001", "b64")]
N_STORED = 2


def as_dtype(base, dtype):
    """The same synthetic patterns in another dtype: uint8 / uint16 as they are, int8 / int16 shifted into the signed
    range, floats from the uint16 values onto [-0.2, 1] (inside the [-1, 1] img_as_uint takes)."""
    base = np.asarray(base)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return ((base.astype(np.float64) / 65535.0) * 1.2 - 0.2).astype(dt)
    if dt == np.int8:
        return (base.astype(np.int16) - 128).astype(np.int8)
    if dt == np.int16:
        return (base.astype(np.int32) - 32768).astype(np.int16)
    return base.astype(dt)


def base_dtype(dtype):
    """The _iq_inputs stack dtype a case dtype derives from."""
    return "uint8" if np.dtype(dtype).itemsize == 1 else "uint16"


def degenerate(dtype):
    """Five 32 x 32 patterns: ordinary, ordinary with one NaN pixel (integer dtypes: one bright pixel), constant,
    all zero, all NaN (integer dtypes: constant at the top of the range)."""
    dt = np.dtype(dtype)
    y, x = np.mgrid[:32, :32]
    base = ((3 * y + 5 * x) % 23).astype(np.float64) * 7 + 20
    if dt.kind == "f":
        s = np.stack([base / 255, base / 255, np.full_like(base, 0.4), np.zeros_like(base), np.full_like(base, np.nan)])
        s[1, 4, 5] = np.nan
        return s.astype(dt)
    top = np.iinfo(dt).max
    s = np.stack([base, base, np.full_like(base, 100.0), np.zeros_like(base), np.full_like(base, float(top))])
    s[1, 4, 5] = 200
    return s.astype(dt)


# what the reference raises (type name and message) for one pattern each
ERRORS = {
    "pattern_1x64": ("uint8", (1, 64), None, 0, 128),   # the default kernel has a 0 entry
    "pattern_64x1": ("uint8", (64, 1), None, 0, 128),
    "float_outside": ("float32", (16, 16), (4, 4), 0, 128),
    "negative_kernel": ("uint8", (16, 16), (-3, 4), 0, 128),
    "nbins_0": ("uint8", (16, 16), (4, 4), 0, 0),
    "nbins_negative": ("uint8", (16, 16), (4, 4), 0, -1),
}


def error_input(name):
    dtype, shape, _, _, _ = ERRORS[name]
    p = (np.arange(shape[0] * shape[1]).reshape(shape) % 200).astype(dtype)
    if name == "float_outside":
        p = (p / 100.0).astype(np.float32)  # up to 1.99
    return p
