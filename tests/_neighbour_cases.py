"""Cases of the neighbour fixture (tests/golden/neighbours.npz, made by tools/gen_neighbour_golden.py): the inputs
(golden arrays and synthetic maps rebuilt at test time with integer arithmetic only), the windows by name, and the
scale of the dot-product bound.  Shared by the generator, tests/test_host_neighbours.py and
tests/test_gpu_neighbours.py."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SYNTH_NAV, SYNTH_SIG, SYNTH_SEED = (6, 7), (24, 20), 11
CONSTANT_POINT = (2, 3)  # of the synthetic map of the dot-product cases


def _hash(n, seed):
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = i * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(31)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(29)
    return x


def synth(dtype, seed=SYNTH_SEED, nav=SYNTH_NAV, sig=SYNTH_SIG):
    """A map of correlated patterns: a shared pattern plus per-point noise, 16-bit integers k, as `dtype` (floats:
    the dyadic values k / 256 - 100, exactly representable, so that sums of small-integer multiples are exact)."""
    n = int(np.prod(nav)) * int(np.prod(sig))
    noise = (_hash(n, seed) >> np.uint64(50)).astype(np.int64).reshape(nav + sig)  # 14 bits
    base = (_hash(int(np.prod(sig)), seed + 1) >> np.uint64(49)).astype(np.int64).reshape(sig)  # 15 bits
    k = base + noise  # < 2**16
    if dtype == "uint8":
        return (k >> 8).astype(np.uint8)
    if dtype == "int8":
        return ((k >> 8) - 128).astype(np.int8)
    if dtype == "uint16":
        return k.astype(np.uint16)
    if dtype == "int16":
        return (k - 32768).astype(np.int16)
    return (k.astype(np.float64) / 256.0 - 100.0).astype(dtype)


def inputs(name):
    if name == "dummy":
        return np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    if name == "dummy1d":
        return inputs("dummy")[0]
    if name == "ni":
        ni = np.load(os.path.join(GOLDEN, "preproc.npz"))["ni"]
        return ni.reshape((3, 3) + ni.shape[-2:])
    if name == "ni1d":
        return np.ascontiguousarray(inputs("ni")[:, 0])  # the first map column (HyperSpy's `inav[0]`)
    if name.startswith("synth_"):
        return synth(name[len("synth_"):])
    if name == "synthc":  # the dot-product map: one constant pattern
        p = synth("uint8").copy()
        p[CONSTANT_POINT] = 7
        return p
    raise KeyError(name)


# averaging windows by name: how `EBSD.average_neighbour_patterns` is called for them; the arrays themselves are in
# the fixture as `win__<name>` (made by the reference's Window)
WINDOWS = {
    "default": dict(window="circular", window_shape=(3, 3)),
    "rect33": dict(window="rectangular", window_shape=(3, 3)),
    "rect23": dict(window="rectangular", window_shape=(2, 3)),
    "w3": dict(window="circular", window_shape=(3,)),
    "gauss": dict(window="gaussian", window_shape=(3, 3), std=2),
    "custom23": dict(window=np.array([[1, 2, 0], [3, 1, 1]])),
    "circ55": dict(window="circular", window_shape=(5, 5)),
}
INTEGER_WINDOWS = [w for w in WINDOWS if w != "gauss"]
AVERAGE_CASES = (
    [(i, w) for i in ("dummy", "ni") for w in ("default", "rect33", "rect23", "w3", "gauss", "custom23")]
    + [("dummy1d", "w3"), ("ni1d", "w3")]
    + [(f"synth_{d}", w) for d in ("uint8", "uint16", "float32", "float64") for w in ("circ55", "custom23")]
    + [("synth_uint8", "gauss")]
)

# dot products: footprints by name (None: the method's default), every flag combination, both dtypes
FOOTPRINTS = {
    "default": None,
    "rect33": dict(window="rectangular", shape=(3, 3)),
    "custom23": np.array([[1, 1, 0], [1, 1, 1]]),
    "w3": dict(window="rectangular", shape=(3,)),
}
DOT_CASES = [("ni", "default"), ("ni", "rect33"), ("ni", "custom23"), ("ni1d", "w3"), ("synthc", "default"),
             ("synthc", "custom23")]
FLAGS = [(True, True), (True, False), (False, True), (False, False)]
DOT_RTOL = 1e-5  # the project's score tolerance and the reference's own test tolerance


def avg_key(inp, win):
    return f"avg__{inp}__{win}"


def dot_key(inp, win, zero_mean, normalize):
    return f"dp__{inp}__{win}__zm{int(zero_mean)}nm{int(normalize)}"


def dot_scale(mat64, normalize):
    """The scale s of the bound |ours - g64| <= 1e-5 s for every entry of float64 matrices nav + window.shape: 1 with
    `normalize`, else sqrt(sum x_q^2 sum x_{q+j}^2) - both sums are origin entries of the matrices; (matrix scale,
    map scale = the largest among the point's neighbours)."""
    mat64 = np.asarray(mat64, dtype=np.float64)
    wshape = mat64.shape[mat64.ndim // 2:]
    nav = mat64.shape[:mat64.ndim // 2]
    origin = tuple(v // 2 for v in wshape)
    if normalize:
        return np.ones(mat64.shape), np.ones(nav)
    c = mat64[(Ellipsis,) + origin]  # sum x_q^2
    s = np.zeros(mat64.shape)
    for q in np.ndindex(*nav):
        for j in np.ndindex(*wshape):
            n = tuple(a + b - o for a, b, o in zip(q, j, origin))
            if all(0 <= v < m for v, m in zip(n, nav)):
                s[q + j] = np.sqrt(c[q] * c[n])
    smap = np.where(np.isnan(mat64), 0.0, s)
    smap[(Ellipsis,) + origin] = 0.0
    return s, smap.reshape(nav + (-1,)).max(axis=-1)
