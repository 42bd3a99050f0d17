"""Cases of the virtual BSE fixture (tests/golden/vbse.npz, made by tools/gen_vbse_golden.py): the inputs (golden arrays
and synthetic maps rebuilt at test time with integer arithmetic only) and the grid / RGB calls by name.  Shared by the
generator, tests/test_host_vbse.py and tests/test_gpu_vbse.py."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SYNTH_NAV, SYNTH_SIG, SYNTH_SEED = (6, 7), (24, 20), 23
DTYPES = ("uint8", "int8", "uint16", "int16", "float32", "float64")


def _hash(n, seed):
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(31)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(29)
    return x


def synth(dtype, seed=SYNTH_SEED, nav=SYNTH_NAV, sig=SYNTH_SIG):
    """A map of patterns whose intensity depends on the map point (grains: a per-point gain on a shared pattern) plus
    noise, 16-bit integers k, as `dtype` (floats: the dyadic values k / 256 - 100)."""
    n = int(np.prod(nav)) * int(np.prod(sig))
    noise = (_hash(n, seed) >> np.uint64(51)).astype(np.int64).reshape(nav + sig)  # 13 bits
    base = (_hash(int(np.prod(sig)), seed + 1) >> np.uint64(50)).astype(np.int64).reshape(sig)  # 14 bits
    gain = (_hash(int(np.prod(nav)), seed + 2) >> np.uint64(62)).astype(np.int64).reshape(nav + (1, 1)) + 1  # 1 ... 4
    k = base * gain // 2 + noise  # < 2**16
    if dtype == "uint8":
        return (k >> 8).astype(np.uint8)
    if dtype == "int8":
        return ((k >> 8) - 128).astype(np.int8)
    if dtype == "uint16":
        return k.astype(np.uint16)
    if dtype == "int16":
        return (k - 32768).astype(np.int16)
    return (k.astype(np.float64) / 256.0 - 100.0).astype(dtype)


def synth_alpha(nav=SYNTH_NAV, seed=SYNTH_SEED):
    """A float alpha map: dyadic values in [0.25, 4.25)."""
    return (_hash(int(np.prod(nav)), seed + 3) >> np.uint64(54)).astype(np.float64).reshape(nav) / 256.0 + 0.25


def inputs(name):
    if name == "dummy":
        return np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    if name == "ni":
        ni = np.load(os.path.join(GOLDEN, "preproc.npz"))["ni"]
        return ni.reshape((3, 3) + ni.shape[-2:])
    if name.startswith("synth_"):
        return synth(name[len("synth_"):])
    raise KeyError(name)


def alpha(name):
    if name is None:
        return None
    if name == "arange9":
        return np.arange(9).reshape((3, 3))
    if name == "arange9_plus10":
        a = np.arange(9).reshape((3, 3))
        a[0] += 10
        return a
    if name == "synth":
        return synth_alpha()
    raise KeyError(name)


# get_images_from_grid: (input, grid shape, dtype_out)
GRID_CASES = (
    [("dummy", (1, 1), "float32"), ("dummy", (1, 1), "float64"), ("dummy", (3, 3), "float32"),
     ("ni", (5, 5), "float32"), ("ni", (5, 5), "uint16"), ("ni", (1, 1), "float64"), ("ni", (13, 7), "float32"),
     ("ni", (10, 10), "int32")]
    + [(f"synth_{d}", g, o) for d in DTYPES for g, o in (((5, 5), "float32"), ((24, 20), "float64"), ((3, 4), "uint8"))]
)

# get_rgb_image: name -> (input, grid shape, r, g, b, keyword arguments; `alpha` by name)
T = [(0, 0), (0, 1), (0, 2)]
RGB_CASES = {
    "ni_default": ("ni", (5, 5), *T, {}),
    "ni_percentiles": ("ni", (5, 5), *T, {"percentiles": (1, 99)}),
    "ni_alpha": ("ni", (5, 5), *T, {"alpha": "arange9"}),
    "ni_alpha10": ("ni", (5, 5), *T, {"alpha": "arange9_plus10"}),
    "ni_two_a": ("ni", (5, 5), [(0, 1), (0, 2)], [(1, 1), (1, 2)], [(2, 1), (2, 2)], {}),
    "ni_two_b": ("ni", (5, 5), [(2, 1), (2, 2)], [(3, 1), (3, 2)], [(4, 1), (4, 2)], {}),
    "ni_u16": ("ni", (5, 5), *T, {"dtype_out": "uint16"}),
    "ni_raw": ("ni", (5, 5), *T, {"normalize": False}),
    "ni_roi": ("ni", (5, 5), ("roi", 0, 0, 10, 10), ("roi", 20, 5, 60, 31), [("roi", 3, 3, 9, 50), (4, 4)], {}),
}
for _d in DTYPES:
    RGB_CASES.update({
        f"synth_{_d}_default": (f"synth_{_d}", (4, 4), (0, 0), (1, 2), (3, 3), {}),
        f"synth_{_d}_u16_mix": (f"synth_{_d}", (4, 5), [(0, 0), (1, 1)], (2, 2), [(3, 4), (0, 3)],
                                {"dtype_out": "uint16", "contrast": 1.5, "add_bright": 20, "alpha": "synth",
                                 "percentiles": (0.5, 99.5)}),
        f"synth_{_d}_raw_alpha": (f"synth_{_d}", (3, 3), (0, 0), (1, 1), (2, 2), {"normalize": False, "alpha": "synth"}),
    })
INTEGER_RGB_CASES = [k for k, v in RGB_CASES.items() if inputs(v[0]).dtype.kind in "iu"]

# the numbers of the reference's tests (tests/test_imaging/test_virtual_bse_imager.py): (wanted mean, atol of
# np.allclose there; None: its default)
KNOWN_RGB_MEAN = {
    "ni_default": (136.481481, None), "ni_percentiles": (134.740740, None), "ni_alpha": (88.5, 0.1),
    "ni_alpha10": (107.9, 0.1), "ni_two_a": (125.1, 0.1), "ni_two_b": (109.0, 0.1),
}
KNOWN_DUMMY_1X1_MEAN = 40.666668


def grid_key(inp, grid, dtype_out):
    return f"grid__{inp}__{grid[0]}x{grid[1]}__{dtype_out}"


def rgb_key(name):
    return f"rgb__{name}"


def close_to_known(mean, want, atol):
    return bool(np.allclose(mean, want) if atol is None else np.allclose(mean, want, atol=atol))
