"""Inputs of the image-quality fixture (tests/golden/image_quality.npz), regenerated at test time: an integer hash of the
pixel index (identical on every NumPy version, nothing random to store) plus a ramp, so that patterns carry some
low-frequency structure as well as noise."""

import numpy as np

SHAPES = [(60, 60), (61, 59), (1, 64), (64, 1), (128, 96), (240, 240), (1001, 1001)]
DTYPES = ["uint8", "uint16", "float32"]
N_PATTERNS = {(240, 240): 3, (1001, 1001): 2}  # else 4


def n_patterns(shape):
    return N_PATTERNS.get(tuple(shape), 4)


def stack(shape, dtype, seed):
    sy, sx = shape
    n = n_patterns(shape)
    i = np.arange(n * sy * sx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(31)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(29)
    noise = (x >> np.uint64(40)).astype(np.float64) / float(1 << 24)  # [0, 1), 24 bits
    y, xx = np.divmod(np.arange(sy * sx) % (sy * sx), sx)
    ramp = (((3 * y + 5 * xx) % 97) / 96.0)[None].repeat(n, 0).ravel()
    v = (0.6 * noise + 0.4 * ramp).reshape(n, sy, sx)
    if dtype == "uint8":
        return np.floor(v * 255).astype(np.uint8)
    if dtype == "uint16":
        return np.floor(v * 65535).astype(np.uint16)
    return (v * 1000 - 300).astype(np.float32)
