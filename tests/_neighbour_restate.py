"""NumPy restatement of the neighbour ops' arithmetic (the reference's `_average_neighbour_patterns` with
`scipy.ndimage.correlate`, and `_neighbour_dot_products` in float64), every rounding explicit, no SciPy.  Test
infrastructure: tests/test_host_neighbours.py pins it to the reference's fixture, tests/test_gpu_neighbours.py compares
the GPU with it where the fixture has no entry.  Deliberately written apart from kikuchipy_amd.pattern._neighbours."""

import numpy as np

DTYPE_RANGE = {np.uint8: (0, 255), np.uint16: (0, 65535), np.int8: (-128, 127), np.int16: (-32768, 32767),
               np.float32: (-1, 1), np.float64: (-1, 1)}


def as_map(patterns, window):
    """(patterns as (ny, nx, sy, sx), window as (wy, wx)): a 1-D map is ny x 1, a 1-D window acts along the rows."""
    p = np.asarray(patterns)
    w = np.asarray(window)
    if p.ndim == 3:
        p = p[:, None]
    return p, w.reshape(w.shape + (1,) * (2 - w.ndim))


def _taps(w):
    wy, wx = w.shape
    for j in range(wy * wx):
        if w.ravel()[j] != 0:
            yield j // wx - wy // 2, j % wx - wx // 2, w.ravel()[j]


def window_sums(window, ny, nx):
    """int64(sum of the coefficients whose neighbour is inside the map), summed in float64 in C order, truncated."""
    out = np.zeros((ny, nx), dtype=np.int64)
    w = np.asarray(window, dtype=np.float64)
    for y in range(ny):
        for x in range(nx):
            acc = 0.0
            for dy, dx, c in _taps(w):
                if 0 <= y + dy < ny and 0 <= x + dx < nx:
                    acc += c
            out[y, x] = int(acc)  # truncation
    return out


def average(patterns, window):
    """`EBSD.average_neighbour_patterns` of (ny, nx, sy, sx) or (n, sy, sx) patterns under `window` (1-D or 2-D)."""
    shape = np.shape(patterns)
    p, w = as_map(patterns, window)
    w = w.astype(np.float64)
    ny, nx = p.shape[:2]
    ws = window_sums(w, ny, nx)
    f = p.astype(np.float32).astype(np.float64)
    out = np.empty(p.shape, dtype=p.dtype)
    omin, omax = DTYPE_RANGE[p.dtype.type]
    for y in range(ny):
        for x in range(nx):
            acc = np.zeros(p.shape[2:], dtype=np.float64)
            for dy, dx, c in _taps(w):
                if 0 <= y + dy < ny and 0 <= x + dx < nx:
                    acc = acc + f[y + dy, x + dx] * c
            a = acc.astype(np.float32).astype(np.float64) / np.float64(ws[y, x])
            imin, imax = a.min(), a.max()
            with np.errstate(invalid="ignore", divide="ignore"):
                r = (a - imin) / float(imax - imin) * (omax - omin) + omin
            if p.dtype.kind in "iu":
                r = np.where(np.isnan(r), -2147483648.0, r).astype(np.int64)  # truncation; 0 / 0: the low bits, 0
            out[y, x] = r.astype(p.dtype)
    return out.reshape(shape)


def _prepared(p, zero_mean, normalize):
    x = p.reshape(p.shape[0], p.shape[1], -1).astype(np.float64)
    if zero_mean:
        x = x - x.mean(axis=-1, keepdims=True)
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            x = x / np.sqrt((x * x).sum(axis=-1, keepdims=True))
    return x


def dot_matrices(patterns, footprint, zero_mean=True, normalize=True):
    """float64 dot product matrices, nav shape + footprint shape; NaN where there is no neighbour."""
    nav = np.shape(patterns)[:-2]
    fshape = np.shape(footprint)
    p, fp = as_map(patterns, np.asarray(footprint) != 0)
    ny, nx = p.shape[:2]
    wy, wx = fp.shape
    x = _prepared(p, zero_mean, normalize)
    out = np.full((ny, nx, wy, wx), np.nan)
    for y in range(ny):
        for xx in range(nx):
            for j in range(wy * wx):
                dy, dx = j // wx - wy // 2, j % wx - wx // 2
                if fp.ravel()[j] and 0 <= y + dy < ny and 0 <= xx + dx < nx:
                    out[y, xx, j // wx, j % wx] = (x[y + dy, xx + dx] * x[y, xx]).sum()
    return out.reshape(nav + fshape)


def adp_from_matrices(mat, nav_dim):
    """nanmean over the window axes with the origin left out; NaN for a point without any dot product."""
    m = np.array(mat, dtype=np.float64)
    wshape = m.shape[nav_dim:]
    m[(Ellipsis,) + tuple(v // 2 for v in wshape)] = np.nan
    flat = m.reshape(m.shape[:nav_dim] + (-1,))
    cnt = (~np.isnan(flat)).sum(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.nansum(flat, axis=-1) / np.where(cnt == 0, np.nan, cnt)
