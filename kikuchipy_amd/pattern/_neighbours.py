"""Neighbour pattern averaging and neighbour dot products on the GPU: the ops whose result at a map point depends on
the patterns around it (csrc/neighbours.hip).

Array-level counterparts of `EBSD.average_neighbour_patterns` (signals/ebsd.py:943-1111, pattern/chunk.py:130-164),
`EBSD.get_neighbour_dot_product_matrices` (signals/ebsd.py:1221-1310) and
`EBSD.get_average_neighbour_dot_product_map` (signals/ebsd.py:1377-1491, signals/util/_map_helper.py).  The patterns
are an array (ny, nx, sy, sx) or (n, sy, sx); on the device a map is always ny x nx points (a 1-D map: nx = 1 and a
window of (wy, 1)).  Several contexts split the map by ROWS: every member uploads its rows plus the halo the window
needs and produces its own rows; the map's border is the only border (`neighbour_row_blocks`).
"""

import warnings

import numpy as np

from kikuchipy_amd.filters import Window
from kikuchipy_amd.pattern import _pattern


def averaging_window(window="circular", window_shape=(3, 3), **kwargs):
    """The window `EBSD.average_neighbour_patterns` averages with (signals/ebsd.py:1010-1013): a valid `Window` is
    copied, anything else goes through `Window(window=window, shape=window_shape, **kwargs)`."""
    if isinstance(window, Window) and window.is_valid:
        return window.copy()
    return Window(window=window, shape=window_shape, **kwargs)


def window_on_map(window, nav_shape):
    """`window` as the 2-D float64 array (wy, wx) the kernels take for a map of `nav_shape`: a 1-D window acts along the
    FIRST navigation axis (`window.reshape(shape + (1,))`, signals/ebsd.py:1024-1025; a 1-D map is ny x 1 points); a
    window with more axes than the map raises (SciPy's correlate refuses it)."""
    w = np.asarray(window, dtype=np.float64)
    if not 1 <= len(nav_shape) <= 2:
        raise ValueError("Signal must have at least one navigation dimension")
    if w.ndim < 1 or w.ndim > len(nav_shape):
        raise ValueError(f"A window of shape {w.shape} has more axes than the map of shape {tuple(nav_shape)}")
    return np.ascontiguousarray(w.reshape(w.shape + (1,) * (2 - w.ndim)))


def neighbour_window_sums(window2d, ny, nx):
    """What `scipy.ndimage.correlate(np.ones((ny, nx), dtype=int), weights=window, mode="constant")` gives: per map
    point the sum of the coefficients whose neighbour lies inside the map - added in float64 in C order over the
    non-zero coefficients, as SciPy does - TRUNCATED to an integer (the reference correlates an integer array)."""
    w = np.asarray(window2d, dtype=np.float64)
    wy, wx = w.shape
    y, x = np.arange(ny)[:, None], np.arange(nx)[None, :]
    acc = np.zeros((ny, nx), dtype=np.float64)
    for j in np.flatnonzero(w.ravel()):
        yy, xx = y + (j // wx - wy // 2), x + (j % wx - wx // 2)
        acc += np.where((yy >= 0) & (yy < ny) & (xx >= 0) & (xx < nx), w.ravel()[j], 0.0)
    return acc.astype(np.int64)


def neighbour_row_blocks(ny, wy, n_members):
    """How a map of `ny` rows is split over `n_members` contexts for a window of `wy` rows: a list of
    (row0, row1, lo, hi) - the member produces the rows [row0, row1) and holds the rows [lo, hi): its own plus a halo
    of wy // 2 rows above and wy - wy // 2 - 1 below, clipped at the map's edge.  Blocks cover the map once; a map with
    fewer rows than members uses fewer members."""
    from kikuchipy_amd.parallel import shard_range

    n = max(1, min(int(n_members), int(ny)))
    above, below = wy // 2, wy - wy // 2 - 1
    out = []
    for i in range(n):
        r0, r1 = shard_range(ny, i, n)
        out.append((r0, r1, max(r0 - above, 0), min(r1 + below, ny)))
    return out


def _as_map(patterns):
    """(flat (ny * nx, sy, sx), ny, nx, navigation shape) of (ny, nx, sy, sx) or (n, sy, sx) patterns."""
    patterns = _pattern.as_patterns(patterns)
    if patterns.ndim not in (3, 4):
        raise ValueError("Signal must have at least one navigation dimension")
    if patterns.dtype.type not in _pattern._SUPPORTED:
        raise ValueError(f"pattern dtype {patterns.dtype} is not supported by the GPU pre-processing kernels")
    nav = patterns.shape[:-2]
    ny, nx = (nav[0], 1) if len(nav) == 1 else nav
    if isinstance(patterns, _pattern.ResidentPatterns):
        return patterns.flat(), int(ny), int(nx), nav
    return np.ascontiguousarray(patterns).reshape((-1,) + patterns.shape[-2:]), int(ny), int(nx), nav


def _run(flat, ny, nx, wy, op, context, device, contexts):
    """`op(ctx, rows held, row0, row1, lo)` -> the array of the rows [row0, row1) (relative to the rows held, which start
    at the map's row `lo`), on one context holding the whole map or on `contexts` block-wise by rows; the parts are
    concatenated along the rows.  Returns (result, or a tuple of results when `op` returns a tuple)."""
    def join(parts):
        if isinstance(parts[0], tuple):
            return tuple(None if p[0] is None else np.concatenate(p, axis=0) for p in zip(*parts))
        return np.concatenate(parts, axis=0)

    if contexts and len(contexts) > 1 and ny > 1:
        from concurrent.futures import ThreadPoolExecutor

        blocks = neighbour_row_blocks(ny, wy, len(contexts))

        def one(job):
            c, (r0, r1, lo, hi) = job
            _pattern._upload(c, flat[lo * nx:hi * nx])
            return op(c, hi - lo, r0 - lo, r1 - lo, lo)

        with ThreadPoolExecutor(len(blocks)) as pool:
            return join(list(pool.map(one, zip(contexts, blocks))))
    if isinstance(flat, _pattern.ResidentPatterns):  # where they are, on their own context
        _pattern._upload(flat.context if context is None else context, flat)
        return join([op(flat.context, ny, 0, ny, 0)])
    ctx = contexts[0] if contexts else _pattern._context(context, device)
    try:
        _pattern._upload(ctx, flat)
        return join([op(ctx, ny, 0, ny, 0)])
    finally:
        if context is None and not contexts:
            ctx.close()


def average_neighbour_patterns_stack(patterns, window="circular", window_shape=(3, 3), *, context=None, device=0,
                                     contexts=None, **kwargs):
    """`EBSD.average_neighbour_patterns` on an array (ny, nx, sy, sx) or (n, sy, sx): every pattern becomes the
    `window`-weighted sum of its neighbours inside the map (as float32), divided by the map point's truncated window
    sum and rescaled to the range of the patterns' dtype; returns a new array of the input's dtype and shape.  Bit-exact
    with the reference's NumPy evaluation for integer-valued windows.  A window of shape (1,) or (1, 1) warns and
    returns a copy; a point whose window sum is 0 raises; a constant averaged pattern becomes 0 (integer dtypes) or NaN
    (float dtypes), as in `rescale_intensity`.  On a single `context` the averaged patterns stay resident."""
    patterns = _pattern.as_patterns(patterns)
    flat, ny, nx, nav = _as_map(patterns)
    win = averaging_window(window, window_shape, **kwargs)
    if win.shape in [(1,), (1, 1)]:
        warnings.warn(f"A window of shape {win.shape} was passed, no averaging is therefore performed")
        if not isinstance(patterns, _pattern.ResidentPatterns):
            return patterns.copy()
        if patterns.keep:
            return patterns
        return patterns.host()
    w = window_on_map(win, nav)
    sums = neighbour_window_sums(w, ny, nx)
    if not sums.all():
        q = np.argwhere(sums == 0)[0]
        raise ValueError(f"The window sum of map point {tuple(int(v) for v in q)} is 0: its average is undefined")

    kept = isinstance(patterns, _pattern.ResidentPatterns) and patterns.keep

    def op(c, rows, row0, row1, lo):
        c.average_neighbour_patterns(rows, nx, w, sums[lo:lo + rows], row0, row1)
        return np.empty(0) if kept else c.get_experimental()[row0 * nx:row1 * nx]

    out = _run(flat, ny, nx, w.shape[0], op, context, device, contexts)
    return patterns if kept else out.reshape(patterns.shape)


def dot_product_window(window, nav_shape):
    """The `Window` of the dot-product methods for a map of `nav_shape`: None gives the nearest neighbours,
    `Window("circular", (3, 3)[:nav_dim])`; the reference takes it as a boolean footprint with as many axes as the map,
    true at its own origin (it fails with an IndexError otherwise)."""
    if not 1 <= len(nav_shape) <= 2:
        raise ValueError("Signal must have at least one navigation dimension")
    if window is None:
        window = Window(window="circular", shape=(3, 3)[:len(nav_shape)])
    elif not isinstance(window, Window):
        window = Window(np.asarray(window))
    if window.ndim != len(nav_shape):
        raise ValueError(f"A window of shape {window.shape} does not have the {len(nav_shape)} axes of the map")
    if not np.asarray(window)[window.origin]:
        raise ValueError(f"The window coefficient at the window's origin {window.origin} is zero: a pattern must be "
                         "part of its own neighbourhood")
    return window


def _dot_dtype(dtype_out):
    dt = np.dtype(dtype_out)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"dtype_out {dt} is not supported: the dot products are float32 or float64")
    return dt


def _dot_products(patterns, window, zero_mean, normalize, dtype_out, matrices, average, context, device, contexts):
    patterns = _pattern.as_patterns(patterns)
    nav = patterns.shape[:-2]
    window = dot_product_window(window, nav)
    dt = _dot_dtype(dtype_out)
    flat, ny, nx, nav = _as_map(patterns)
    fp = window_on_map(np.asarray(window) != 0, nav) != 0

    def op(c, rows, row0, row1, lo):
        return c.neighbour_dot_products(rows, nx, fp, zero_mean, normalize, dt, row0, row1, matrices, average)

    mat, adp = _run(flat, ny, nx, fp.shape[0], op, context, device, contexts)
    return (None if mat is None else mat.reshape(nav + window.shape)), (None if adp is None else adp.reshape(nav))


def neighbour_dot_product_matrices(patterns, window=None, zero_mean=True, normalize=True, dtype_out="float32", *,
                                   context=None, device=0, contexts=None):
    """`EBSD.get_neighbour_dot_product_matrices` on an array (ny, nx, sy, sx) or (n, sy, sx): per map point the dot
    products of its pattern with the neighbours the boolean `window` selects, shape nav_shape + window.shape of
    `dtype_out` (float32 / float64); NaN where the window is false or the neighbour lies outside the map, the pattern's
    own sum of squares at the window's origin.  Patterns are centred (`zero_mean`) and divided by their norm
    (`normalize`) first; all sums run in float64."""
    return _dot_products(patterns, window, zero_mean, normalize, dtype_out, True, False, context, device, contexts)[0]


def average_neighbour_dot_product_map(patterns, window=None, zero_mean=True, normalize=True, dtype_out="float32", *,
                                      context=None, device=0, contexts=None):
    """`EBSD.get_average_neighbour_dot_product_map` on an array: per map point the mean of the non-NaN dot products
    with its neighbours (`neighbour_dot_product_matrices` without the origin), NaN for a point without any; shape
    nav_shape of `dtype_out`."""
    return _dot_products(patterns, window, zero_mean, normalize, dtype_out, False, True, context, device, contexts)[1]


def average_dot_product_map_from_matrices(dp_matrices, window, nav_dim):
    """The average map of given dot product matrices on the host (signals/ebsd.py:1432-1441): the entry at the
    window's origin set to NaN, `nanmean` over the window axes."""
    nan_slices = [slice(None) for _ in range(nav_dim)]
    nan_slices += [slice(i, i + 1) for i in window.origin]
    dp_matrices2 = np.array(dp_matrices, copy=True)
    dp_matrices2[tuple(nan_slices)] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # a point without neighbours: mean of an empty slice, NaN
        return np.nanmean(dp_matrices2, axis=1 if nav_dim == 1 else (2, 3))
