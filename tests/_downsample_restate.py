"""NumPy restatements of what csrc/downsample.hip and the dynamic-background kernel of csrc/preproc.hip compute, pinned
to the reference's own results in tests/golden/downsample.npz by tests/test_host_downsample.py.

`downsample`: the reference's _bin2d / _downsample2d (pattern/_pattern.py:776-807) as its py_func evaluates them under
NumPy 1.26 - bit for bit.  `get_dynamic_background`: EBSD.get_dynamic_background (signals/ebsd.py:698-803) with the FFT
filter replaced by the float64 correlation it equals up to its float32 round-off, and scipy.ndimage.gaussian_filter by
its two 1-D passes in SciPy's own order of operations (bit for bit), each stored in the output dtype.  SciPy 1.7.1's
double -> integer store is the C conversion, truncation toward zero, in both passes (probed on uint8 / int8 / int16 rows with values at .25, .5, .75 on either side
of 0: 1.75 -> 1, 9.5 -> 9, -1.75 -> -1, -9.5 -> -9, -0.25 -> 0; a uint8 / int8 / int16 gaussian_filter equals two
truncating passes exactly and differs from a single final truncation)."""

import numpy as np

DTYPE_RANGE = {np.uint8: (0, 255), np.int8: (-128, 127), np.uint16: (0, 65535), np.int16: (-32768, 32767),
               np.float32: (-1, 1), np.float64: (-1, 1)}


def astype(v, dtype):
    """ndarray.astype(dtype) on x86-64 (tests/_intensity_restate.py: astype): floats round to nearest; integers truncate
    to int32 (NaN and values outside int32 give INT32_MIN), then keep the low bits."""
    dt = np.dtype(dtype)
    v = np.asarray(v)
    if dt.kind == "f" or v.dtype.kind in "iu":
        return v.astype(dt)
    with np.errstate(invalid="ignore"):
        ok = (v >= -2147483648.0) & (v < 2147483648.0)
        i = np.where(ok, np.trunc(np.where(ok, v, 0)), -2147483648).astype(np.int64)
    return i.astype(dt)


def bin2d(p, factor):
    """_bin2d: every binned pixel the float32 sum of its factor x factor pixels added one by one, rows outer, columns
    inner.  Adding the strided slices in that order performs the same float32 additions per pixel."""
    p = np.asarray(p, dtype=np.float32)
    b = np.zeros((p.shape[0] // factor, p.shape[1] // factor), dtype=np.float32)
    with np.errstate(all="ignore"):
        for rr in range(factor):
            for cc in range(factor):
                b = b + p[rr::factor, cc::factor]
    return b


def downsample(p, factor, dtype_out=None):
    """_downsample2d of one pattern with the range of `dtype_out` (default: the pattern's dtype)."""
    p = np.asarray(p)
    dt = p.dtype if dtype_out is None else np.dtype(dtype_out)
    omin, omax = DTYPE_RANGE[dt.type]
    with np.errstate(all="ignore"):
        b = bin2d(astype(p, np.float32), factor)
        imin, imax = np.min(b), np.max(b)  # NaN propagates
        r = (b - imin) / np.float32(imax - imin)
        r = r * np.float32(omax - omin) + np.float32(omin)
    assert r.dtype == np.float32
    return astype(r, dt)


def downsample_stack(stack, factor, dtype_out=None):
    stack = np.asarray(stack)
    flat = stack.reshape((-1,) + stack.shape[-2:])
    out = np.stack([downsample(p, factor, dtype_out) for p in flat])
    return out.reshape(stack.shape[:-2] + out.shape[-2:])


def gaussian_window(filter_domain, std, truncate):
    """(taps, centre, numpy pad mode): out[a] = sum_u taps[u] in[a + u - centre]."""
    if filter_domain == "frequency":
        n = int(truncate * std)
        x = np.arange(n) - (n - 1) / 2.0
        w = np.exp(-0.5 * (x / std) ** 2)
        return w / w.sum(), n - 1 - (n - 1) // 2, "edge"
    if filter_domain == "spatial":
        r = int(truncate * std + 0.5)
        x = np.arange(-r, r + 1)
        w = np.exp(-0.5 / (std * std) * x ** 2)
        return w / w.sum(), r, "symmetric"  # scipy's 'reflect'
    raise ValueError(f"{filter_domain} must be either of ['frequency', 'spatial']")


def correlate1d(x, taps, centre, mode, axis, symmetric=False):
    """float64 correlation along `axis` of (..., sy, sx).  `symmetric`: in the order of SciPy's correlate1d for a
    symmetric kernel of odd length, which decides the last bit and so where a truncation falls:
    t = in[l] w[r]; then for d = r ... 1: t += (in[l - d] + in[l + d]) w[r - d], every operation rounded."""
    x = np.asarray(x, dtype=np.float64)
    n = len(taps)
    pad = [(0, 0)] * x.ndim
    pad[axis] = (centre, n - 1 - centre)
    xp = np.pad(x, pad, mode=mode)
    length = x.shape[axis]

    def at(u):
        return np.take(xp, np.arange(u, u + length), axis=axis)

    if symmetric:
        r = centre
        assert n == 2 * r + 1
        out = at(r) * taps[r]
        for d in range(r, 0, -1):
            out = out + (at(r - d) + at(r + d)) * taps[r - d]
        return out
    out = np.zeros_like(x)
    for u in range(n):
        out += taps[u] * at(u)
    return out


def get_dynamic_background(stack, filter_domain="frequency", std=None, truncate=4.0, dtype_out=None):
    stack = np.asarray(stack)
    dt = stack.dtype if dtype_out is None else np.dtype(dtype_out)
    if std is None:
        std = stack.shape[-1] / 8
    taps, centre, mode = gaussian_window(filter_domain, std, truncate)
    x = astype(stack, dt)  # the cast comes first
    with np.errstate(all="ignore"):
        if filter_domain == "frequency":
            y = correlate1d(x.astype(np.float32), taps, centre, mode, -2)
            y = correlate1d(y, taps, centre, mode, -1)
            return astype(y.astype(np.float32), dt)
        y = astype(correlate1d(x, taps, centre, mode, -2, True), dt)
        return astype(correlate1d(y, taps, centre, mode, -1, True), dt)
