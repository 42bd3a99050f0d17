"""Selecting data from an `EBSD` signal: what `EBSD.inav` / `isig` / `crop` / `crop_signal` / `extract_grid` share.

Everything here is host arithmetic on shapes.  A selection is translated into the arguments of
`_lib.Context.select_patterns` (kpdi_select_patterns): the flat indices of the chosen patterns and, per detector axis,
`(first, step, count)`.  A host-backed signal applies the same numbers with NumPy indexing.

`grid_indices` restates signals/util/array_tools.py:21-107 of the reference.
"""

import numbers

import numpy as np


def grid_indices(grid_shape, nav_shape, return_spacing=False):
    """Indices of a grid evenly spaced in a larger grid of one or two dimensions: an array of shape
    `(ndim,) + the grid's shape` into the grid spanned by `nav_shape` (rows first), and the spacing per dimension with
    `return_spacing`.  The spacing is ceil(nav / (grid + 1)); every spacing-th point except the first of each axis is
    taken and the set is centred, so the grid that comes back can be smaller than the one asked for."""
    if isinstance(grid_shape, (int, np.integer)):
        grid_shape = (int(grid_shape),)
    if isinstance(nav_shape, (int, np.integer)):
        nav_shape = (int(nav_shape),)
    ndim = len(nav_shape)
    if ndim != len(grid_shape):
        raise ValueError("`grid_shape` and `nav_shape` must both signify either a 1D or 2D grid")
    nav = np.array(nav_shape)
    spacing = np.ceil(nav / (np.array(grid_shape) + 1)).astype(int)
    flat = np.arange(int(np.prod(nav_shape))).reshape(nav_shape)
    taken = flat[tuple(slice(None, None, int(s)) for s in spacing)][(slice(1, None),) * ndim]
    idx = np.stack(np.unravel_index(taken, nav_shape))
    first, last = idx[(slice(None),) + (0,) * ndim], idx[(slice(None),) + (-1,) * ndim]
    shift = (first - (nav - last)) // 2
    for axis in range(ndim):
        idx[axis] -= shift[axis]
    return (idx, spacing) if return_spacing else idx


def axis_selection(key, size, what, allow_int=True):
    """One int or slice on an axis of `size` points, read as NumPy reads it: (first, step, count, dropped)."""
    if isinstance(key, (bool, np.bool_)) or (isinstance(key, (numbers.Real, np.floating)) and
                                             not isinstance(key, (numbers.Integral, np.integer))):
        raise TypeError(f"{what} index {key!r}: only integers and slices of integers select data here (indexing by axis "
                        "value is not implemented)")
    if isinstance(key, (numbers.Integral, np.integer)):
        if not allow_int:
            raise ValueError(f"{what} index {int(key)}: an integer would remove a signal axis, and a pattern has two; "
                             f"use a slice ({int(key)}:{int(key) + 1})")
        i = int(key)
        if i < -size or i >= size:
            raise IndexError(f"{what} index {i} is out of bounds for an axis of size {size}")
        return (i + size if i < 0 else i), 1, 1, True
    if not isinstance(key, slice):
        raise TypeError(f"{what} index {key!r}: only integers and slices select data here")
    for v in (key.start, key.stop, key.step):
        if v is not None and not isinstance(v, (numbers.Integral, np.integer)):
            raise TypeError(f"{what} slice {key!r}: only integers select data here (indexing by axis value is not "
                            "implemented)")
    if key.step is not None and key.step < 1:
        raise ValueError(f"{what} slice {key!r}: the step must be positive")
    first, stop, step = key.indices(size)
    count = len(range(first, stop, step))
    if count < 1:
        raise IndexError(f"{what} slice {key!r} selects nothing from an axis of size {size}")
    return first, step, count, False


def _keys(key, ndim, what):
    key = key if isinstance(key, tuple) else (key,)
    if len(key) > ndim:
        raise IndexError(f"too many indices: {len(key)} for {ndim} {what} axes")
    return key + (slice(None),) * (ndim - len(key))


def navigation_selection(nav_shape_rc, key):
    """`s.inav[key]` on a map of `nav_shape_rc` (array order): `key` in HyperSpy's (x, y) order.  Returns (flat indices
    of the chosen patterns as int64 in the new map's order, the new navigation shape in array order, and per ARRAY axis
    the (first, step, count, dropped) the key gave it)."""
    nav = tuple(int(n) for n in nav_shape_rc)
    if not nav:
        raise IndexError("the signal has no navigation axes to index")
    keys = _keys(key, len(nav), "navigation")[::-1]  # array order
    axes = [axis_selection(k, n, "navigation") for k, n in zip(keys, nav)]
    picks = [np.arange(f, f + s * c, s, dtype=np.int64)[:c] for f, s, c, _ in axes]
    flat = picks[0] if len(nav) == 1 else (picks[0][:, None] * nav[1] + picks[1][None, :]).ravel()
    new_nav = tuple(c for _, _, c, dropped in axes if not dropped)
    return np.ascontiguousarray(flat, dtype=np.int64), new_nav, axes


def signal_selection(sig_shape_rc, key):
    """`s.isig[key]` on patterns of `sig_shape_rc` = (rows, columns): `key` in HyperSpy's (x, y) = (columns, rows)
    order.  Returns ((first, step, count) of the rows, the same of the columns)."""
    sy, sx = (int(n) for n in sig_shape_rc)
    kx, ky = _keys(key, 2, "signal")
    rows = axis_selection(ky, sy, "signal", allow_int=False)[:3]
    cols = axis_selection(kx, sx, "signal", allow_int=False)[:3]
    return rows, cols


# EBSD.crop: the axes in HyperSpy's order - navigation axes first (x, y), then the signal axes (dx, dy) - mapped to
# ("navigation" | "signal", position in the (x, y) key)
def crop_axis(axis, nav_dim):
    names = ["x", "y"][:nav_dim] + ["dx", "dy"]
    if isinstance(axis, str):
        if axis not in names:
            raise ValueError(f"axis {axis!r} is none of {names}")
        i = names.index(axis)
    elif isinstance(axis, (numbers.Integral, np.integer)) and not isinstance(axis, bool):
        i = int(axis)
        if i < -len(names) or i >= len(names):
            raise ValueError(f"axis {i} is out of range for the {len(names)} axes {names}")
        i %= len(names)
    else:
        raise TypeError(f"axis {axis!r}: an int or one of {names}")
    return ("navigation", i) if i < nav_dim else ("signal", i - nav_dim)
