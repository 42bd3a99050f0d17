"""Cases, exact restatement and per-value tolerance of the axis reductions (EBSD.sum / mean / max / min / std / var,
csrc/reduce.hip) for tests/test_host_reduce.py and tests/test_gpu_reduce.py.

The restatement works on the reduction as rows: the kept axes in front, the reduced ones flattened (`rows`).  Integer
patterns are restated exactly - int64 sums, Python integers and `fractions.Fraction` for the variance -, float
patterns in `np.longdouble` (64-bit significand: its own error, `LD`, is part of the bound).  The tolerances are the
ones DESIGN.md section 24 derives, with u = 2^-53 and n the number of reduced values:

- integer sum / mean / max / min: 0, and the bits of NumPy;
- integer var: the device takes D = n sum x^2 - (sum x)^2 exactly and rounds four times on the way to D / n^2 (two
  conversions and an addition that join the halves of D, two divisions): g4 = 4u / (1 - 4u), relative; integer std:
  the square root halves that and adds its own error, at most one ulp = 2u: (g4 / 2 + 2u) (1 + g4), relative;
- float sum: half an ulp of the output dtype at the exact value + (n - 1) u sum|x|; float mean: the same / n;
- float var: the device's mean is off by at most dm = (n - 1) u sum|x| / n + u |mean|, which adds dm^2 to the mean
  squared deviation (sum (x - c)^2 = sum (x - mean)^2 + n (mean - c)^2); every term then carries three roundings, the sum
  n - 1, the division one: E = dm^2 + (n + 3) u (var + dm^2), and half an ulp of the output at the exact value;
- float std: |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), the square root's own ulp (2u, relative) and
  half an ulp of the output.
Non-finite exact values (a NaN or an infinity in the window) must come back as they are.
"""

import itertools
from fractions import Fraction

import numpy as np

OPS = ("sum", "mean", "max", "min", "std", "var")
DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.float32, np.float64)
SHAPES = {4: (5, 6, 7, 9), 3: (6, 7, 9), 2: (7, 9)}  # odd, no two axes alike, more than one workgroup of outputs in 4-D
U = 2.0 ** -53
G4 = 4 * U / (1 - 4 * U)
LD = float(np.finfo(np.longdouble).eps)


def subsets(ndim):
    """Every non-empty set of array axes."""
    return [c for k in range(1, ndim + 1) for c in itertools.combinations(range(ndim), k)]


def hyperspy_axes(array_axes, navigation_dimension):
    """The HyperSpy indices (navigation first, each group in (x, y) order) of array axes."""
    nd = navigation_dimension
    order = list(range(nd))[::-1] + [nd + 1, nd]
    return tuple(order.index(a) for a in array_axes)


def result_dtype(dtype, op):
    """The table of the issue (NumPy 2.2.6)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f" or op in ("max", "min"):
        return dtype
    if op == "sum":
        return np.dtype(np.uint64 if dtype.kind == "u" else np.int64)
    return np.dtype(np.float64)


def make_data(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)
    return (rng.standard_normal(shape) * 50 + 20).astype(dtype)


def rows(data, axes):
    """(outputs, reduced values) view of the reduction and the shape of the result."""
    axes = sorted({a % data.ndim for a in axes})
    kept = [k for k in range(data.ndim) if k not in axes]
    n = int(np.prod([data.shape[k] for k in axes]))
    return np.transpose(data, kept + axes).reshape(-1, n), tuple(data.shape[k] for k in kept)


def ulp(value, dtype):
    """The spacing of `dtype` in the binade of |value| (the smallest subnormal below the normal range)."""
    info = np.finfo(dtype)
    _, e = np.frexp(np.abs(np.asarray(value, dtype=np.longdouble)))
    return np.ldexp(np.longdouble(1), np.maximum(e - info.nmant - 1, info.minexp - info.nmant))


def restate(data, op, axes):
    """(exact, tolerance) per output value, in the result's shape.  Integer var / std: `Fraction`s (the variance and its
    relative tolerance - `check` compares squares for std); everything else: longdouble / the result dtype."""
    r, shape = rows(np.asarray(data), axes)
    n = r.shape[1]
    kind = r.dtype.kind
    out = result_dtype(r.dtype, op)
    if op in ("max", "min"):
        x = r.astype(np.longdouble) if kind == "f" else r.astype(np.int64)
        v = x.max(axis=1) if op == "max" else x.min(axis=1)  # (NaN propagates in NumPy's max / min)
        return v.astype(out).reshape(shape), np.zeros(shape)
    if kind in "iu":
        s1 = r.astype(np.int64).sum(axis=1)
        if op == "sum":
            return s1.astype(out).reshape(shape), np.zeros(shape)
        if op == "mean":
            return (s1.astype(np.float64) / n).reshape(shape), np.zeros(shape)
        s2 = (r.astype(np.int64) ** 2).sum(axis=1)
        var = np.empty(len(s1), dtype=object)
        for i in range(len(s1)):
            var[i] = Fraction(n * int(s2[i]) - int(s1[i]) ** 2, n * n)
        rel = G4 if op == "var" else (G4 / 2 + 2 * U) * (1 + G4)
        return var.reshape(shape), np.full(shape, rel)
    x = r.astype(np.longdouble)
    with np.errstate(invalid="ignore", over="ignore"):
        s, a = x.sum(axis=1), np.abs(x).sum(axis=1)
        own = n * LD * a  # the restatement's own summation error
        if op == "sum":
            return s.reshape(shape), (ulp(s, out) / 2 + (n - 1) * U * a + own).reshape(shape)
        mean = s / n
        if op == "mean":
            return mean.reshape(shape), (ulp(mean, out) / 2 + ((n - 1) * U * a + own) / n).reshape(shape)
        d = x - mean[:, None]
        var = (d * d).sum(axis=1) / n
        dm = ((n - 1) * U * a + own) / n + U * np.abs(mean)
        e = dm * dm + (n + 3) * U * (var + dm * dm) + n * LD * var
        if op == "var":
            return var.reshape(shape), (e + ulp(var, out) / 2).reshape(shape)
        std = np.sqrt(var)
        with np.errstate(divide="ignore"):
            shift = np.where(std > 0, np.minimum(e / std, np.sqrt(e)), np.sqrt(e))
        return std.reshape(shape), (shift + 2 * U * std + ulp(std, out) / 2).reshape(shape)


def check(got, data, op, axes):
    """Hold `got` to the restatement: shape, dtype, and every value inside its tolerance.  Returns the largest
    error / tolerance met (0 where the tolerance is 0 and the value is exact); raises AssertionError otherwise."""
    data = np.asarray(data)
    got = np.asarray(got)
    exact, tol = restate(data, op, axes)
    assert got.shape == exact.shape, (got.shape, exact.shape)
    assert got.dtype == result_dtype(data.dtype, op), (got.dtype, result_dtype(data.dtype, op))
    if exact.dtype == object:  # integer var / std
        worst = 0.0
        for g, v, t in zip(got.ravel(), exact.ravel(), tol.ravel()):
            g, t = Fraction(float(g)), Fraction(float(t))
            if op == "std":
                lo, hi, g = v * (1 - t) ** 2, v * (1 + t) ** 2, g * g
            else:
                lo, hi = v * (1 - t), v * (1 + t)
            assert lo <= g <= hi, (op, float(g), float(v), float(t))
            if v:
                worst = max(worst, float(abs(g - v) / (v * t)) / (2 if op == "std" else 1))
        return worst
    if data.dtype.kind in "iu" or op in ("max", "min"):
        same = (got == exact) | ((got != got) & (exact != exact))
        assert same.all(), (op, got.ravel()[~same.ravel()][:4], exact.ravel()[~same.ravel()][:4])
        return 0.0
    finite = np.isfinite(exact)
    assert np.array_equal(np.isnan(got), np.isnan(exact)), (op, "NaN where the exact value has none, or none where it has")
    inf = np.isinf(exact)
    assert np.array_equal(got[inf].astype(np.longdouble), exact[inf]), (op, "infinities")
    err = np.abs(got[finite].astype(np.longdouble) - exact[finite])
    ratio = err / tol[finite]
    assert (err <= tol[finite]).all(), (op, data.dtype, axes, float(ratio.max()))
    return float(ratio.max()) if ratio.size else 0.0
