"""What is done with the orientations that indexing and refinement return: disorientation angles, reduction to the
fundamental zone and kernel average misorientation (KAM) maps, under the proper operations of the point groups
(csrc/orientations.hip, csrc/orientations_plan.h).

Conventions.  Quaternions are (a, b, c, d); an orientation g maps lab to crystal (orix's convention, what
`DictionaryXmap.rotations` and `RefinementResult.rotations` hold).  A point group gives the operations
`S = sampling.rotation_group_operations(sampling.rotation_group_name(point_group))` - no second table of groups, the
same settings; the ten groups with improper operations but no inversion centre are refused with that module's
`ValueError`.  The equivalents of g are s g, s in S.

  * the disorientation angle w(g1, g2; S1, S2) is the smallest rotation angle of (s2 g2)(s1 g1)^-1.  The scalar part of
    that product is the 4-D dot product (s1 g1) . (s2 g2), so the search is max |(s1 g1) . (s2 g2)|; the winning product
    is evaluated again and the angle is 2 atan2(|v|, |w|) (2 acos of the maximum is 1 % off at 1e-7 rad).  For S1 = S2
    one side's equivalents suffice: left multiplication by a unit quaternion keeps the dot product,
    (s1 g1) . (s2 g2) = g1 . (s1^-1 s2 g2), and s1^-1 s2 runs over the group.  `point_group="1"` is orix's
    `Rotation.angle_with`, equal groups are `Orientation.angle_with`;
  * zone reduction takes the equivalent with the largest |a| (the lowest operation index among bitwise equal maxima)
    with a >= 0, a half turn with its first non-zero component positive (the sign rule of `rotation_group_operations`):
    it lies in the closed zone of `fundamental_zone_faces`, both being the Voronoi cell of the identity;
  * KAM is, per map point, the mean angle to the neighbours under a window.

Inputs of any real dtype are converted to float64 and normalised; a row with a non-finite component or a zero norm
gives NaN.  With neither `device` nor `context` the functions run on the host in NumPy float64 by the same formula (as
`get_sample_fundamental` offers both paths); `device` (a GPU's number) or `context` (a `Context`) runs the kernels."""

import numpy as np

from kikuchipy_amd import sampling

__all__ = ["disorientation_angle", "disorientation_angle_outer", "reduce_to_fundamental_zone",
           "kernel_average_misorientation_map"]

_HOST_ROWS = 1 << 16  # pairs evaluated at once on the host


def _quaternions(rotations):
    """(..., 4) float64 of an array, or of an object with `.rotations` (this package's result holders) or `.data` (an
    orix object)."""
    for name in ("rotations", "data"):
        if not isinstance(rotations, np.ndarray) and hasattr(rotations, name):
            rotations = getattr(rotations, name)
    q = np.asarray(rotations)
    if q.dtype.kind not in "fiub":
        raise ValueError(f"rotations of dtype {q.dtype}: a real dtype is needed")
    q = q.astype(np.float64, copy=False)
    if q.ndim < 1 or q.shape[-1] != 4:
        raise ValueError(f"rotations of shape {q.shape}: the last axis holds the 4 quaternion components")
    return q


def _operations(point_group, point_group2=None):
    """(ops1, ops2) as the kernels take them: equal groups give the identity alone on the first side."""
    g1 = sampling.rotation_group_name(point_group)
    g2 = g1 if point_group2 is None else sampling.rotation_group_name(point_group2)
    ops2 = sampling.rotation_group_operations(g2)
    ops1 = sampling.rotation_group_operations("1") if g1 == g2 else sampling.rotation_group_operations(g1)
    return ops1, ops2


def _context(device, context):
    if device is None and context is None:
        return None, False
    if context is not None:
        return context, False
    from kikuchipy_amd import _lib

    return _lib.Context(device), True


# ---- the host path: the formula of csrc/orientations_plan.h in NumPy float64 ---------------------------------------------
def _normalise(q):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])
        ok = (n > 0) & (n <= np.finfo(np.float64).max)
        return np.where(ok[..., None], q / np.where(ok, n, 1.0)[..., None], np.nan)


def _product(p, q):
    """Hamilton product, the operation order of ori_product."""
    p0, p1, p2, p3 = (p[..., k] for k in range(4))
    q0, q1, q2, q3 = (q[..., k] for k in range(4))
    return np.stack([p0 * q0 - p1 * q1 - p2 * q2 - p3 * q3, p0 * q1 + p1 * q0 + p2 * q3 - p3 * q2,
                     p0 * q2 - p1 * q3 + p2 * q0 + p3 * q1, p0 * q3 + p1 * q2 - p2 * q1 + p3 * q0], axis=-1)


def _angle(e1, e2):
    r = _product(e2, e1 * np.array([1.0, -1.0, -1.0, -1.0]))
    return 2.0 * np.arctan2(np.sqrt(r[..., 1] * r[..., 1] + r[..., 2] * r[..., 2] + r[..., 3] * r[..., 3]), np.abs(r[..., 0]))


def _pair_angles_host(g1, g2, ops1, ops2):
    """Angles (radians) of NORMALISED (P, 4) rows, pair by pair."""
    best = np.full(g1.shape[0], -1.0)
    b1, b2 = g1.copy(), g2.copy()
    with np.errstate(invalid="ignore"):
        for i, s1 in enumerate(ops1):
            e1 = _product(s1, g1)
            for j, s2 in enumerate(ops2):
                e2 = _product(s2, g2)
                d = np.abs(e1[:, 0] * e2[:, 0] + e1[:, 1] * e2[:, 1] + e1[:, 2] * e2[:, 2] + e1[:, 3] * e2[:, 3])
                take = d > best
                if i == 0 and j == 0:
                    take = np.ones_like(take)
                best = np.where(take, d, best)
                b1 = np.where(take[:, None], e1, b1)
                b2 = np.where(take[:, None], e2, b2)
        return _angle(b1, b2)


def _pairs_host(q1, q2, shape, ops1, ops2):
    a = np.broadcast_to(q1, shape + (4,)).reshape(-1, 4)
    b = np.broadcast_to(q2, shape + (4,)).reshape(-1, 4)
    out = np.empty(a.shape[0], dtype=np.float64)
    for lo in range(0, a.shape[0], _HOST_ROWS):
        hi = min(lo + _HOST_ROWS, a.shape[0])
        out[lo:hi] = _pair_angles_host(_normalise(a[lo:hi]), _normalise(b[lo:hi]), ops1, ops2)
    return out.reshape(shape)


def _scale(angles, degrees):
    return angles * 57.29577951308232 if degrees else angles


def _broadcast_strides(shape_in, shape_out):
    """Strides in rows of a C-contiguous (shape_in, 4) array viewed as `shape_out` leading axes, 0 where broadcast."""
    pad = (1,) * (len(shape_out) - len(shape_in)) + tuple(shape_in)
    strides, step = [], 1
    for n in reversed(pad):
        strides.append(step if n != 1 else 0)
        step *= n
    strides = strides[::-1]
    return [0 if n_out == 1 else s for s, n_out in zip(strides, shape_out)]


# ---- the public functions -----------------------------------------------------------------------------------------------
def disorientation_angle(rotations1, rotations2, point_group="1", point_group2=None, degrees=False, *, device=None,
                         context=None):
    """The disorientation angle between `rotations1` and `rotations2`, element by element with NumPy broadcasting of
    the leading axes ((M, k, 4) against (M, 1, 4): every top-k candidate to the best): float64 of the broadcast shape,
    radians or `degrees`.  `point_group` is the first set's group, `point_group2` the second's (None: the same);
    `point_group="1"` is orix's `Rotation.angle_with`, equal groups are `Orientation.angle_with`.  The arguments take an
    (..., 4) array or any object with `.rotations` or `.data`."""
    q1, q2 = _quaternions(rotations1), _quaternions(rotations2)
    ops1, ops2 = _operations(point_group, point_group2)
    try:
        shape = tuple(int(v) for v in np.broadcast_shapes(q1.shape[:-1], q2.shape[:-1]))
    except ValueError:
        raise ValueError(f"rotations of shapes {q1.shape} and {q2.shape} do not broadcast") from None
    if int(np.prod(shape, dtype=np.int64)) == 0:
        return np.empty(shape, dtype=np.float64)
    ctx, own = _context(device, context)
    if ctx is None:
        return _scale(_pairs_host(q1, q2, shape, ops1, ops2), degrees)
    try:
        from kikuchipy_amd import _lib

        if len(shape) > _lib.ORIENTATION_MAX_DIMS:
            raise ValueError(f"{len(shape)} leading axes: at most {_lib.ORIENTATION_MAX_DIMS}")
        return ctx.orientation_pairs(q1, q2, shape, _broadcast_strides(q1.shape[:-1], shape),
                                     _broadcast_strides(q2.shape[:-1], shape), ops1, ops2, degrees)
    finally:
        if own:
            ctx.close()


def disorientation_angle_outer(rotations1, rotations2=None, point_group="1", point_group2=None, degrees=False,
                               dtype_out="float64", *, device=None, context=None):
    """The (N, M) disorientation angles of every orientation of `rotations1` (flattened to (N, 4)) with every one of
    `rotations2` ((M, 4); None: the first set with itself) - the input of orientation clustering and of texture
    comparisons.  `dtype_out` is float64 or float32 (the float64 angle rounded once).  On the device one tiled float64
    kernel; output that does not fit in free device memory is walked in passes of rows."""
    dt = np.dtype(dtype_out)
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError(f"dtype_out {dt} is not supported: the angles are float64 or float32")
    q1 = _quaternions(rotations1).reshape(-1, 4)
    q2 = q1 if rotations2 is None else _quaternions(rotations2).reshape(-1, 4)
    ops1, ops2 = _operations(point_group, point_group2)
    n, m = q1.shape[0], q2.shape[0]
    if n == 0 or m == 0:
        return np.empty((n, m), dtype=dt)
    ctx, own = _context(device, context)
    if ctx is None:
        out = np.empty((n, m), dtype=dt)
        rows = max(1, _HOST_ROWS // m)
        for lo in range(0, n, rows):
            hi = min(lo + rows, n)
            out[lo:hi] = _scale(_pairs_host(q1[lo:hi, None, :], q2[None, :, :], (hi - lo, m), ops1, ops2), degrees)
        return out
    try:
        return ctx.orientation_outer(q1, q2, ops1, ops2, degrees, dt)
    finally:
        if own:
            ctx.close()


def _reduce_host(q, ops):
    g = _normalise(q)
    bad = np.isnan(g[:, 0])
    best = np.full(g.shape[0], -1.0)
    out, index = g.copy(), np.zeros(g.shape[0], dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for j, s in enumerate(ops):
            e = _product(s, g)
            take = np.abs(e[:, 0]) > best
            best = np.where(take, np.abs(e[:, 0]), best)
            out = np.where(take[:, None], e, out)
            index = np.where(take, j, index).astype(np.int32)
        lead = np.zeros(g.shape[0])
        for k in (3, 2, 1, 0):
            lead = np.where(out[:, k] != 0, out[:, k], lead)
        out = np.where((lead < 0)[:, None], -out, out)
    out[bad] = np.nan
    index[bad] = -1
    return out, index


def reduce_to_fundamental_zone(rotations, point_group, return_index=False, *, device=None, context=None):
    """Every orientation's equivalent s g in the closed fundamental zone of `point_group`'s rotation group
    (`sampling.fundamental_zone_faces`): the one with the largest |a|, the lowest operation index among equal maxima,
    returned with a >= 0.  Float64 of the input's shape; with `return_index` also the index of s in
    `sampling.rotation_group_operations` (int32, -1 for NaN rows)."""
    q = _quaternions(rotations)
    ops = sampling.rotation_group_operations(sampling.rotation_group_name(point_group))
    flat = q.reshape(-1, 4)
    ctx, own = _context(device, context)
    if flat.shape[0] == 0:
        out, index = flat.copy(), np.empty(0, dtype=np.int32)
    elif ctx is None:
        out, index = _reduce_host(flat, ops)
    else:
        try:
            out, index = ctx.orientation_reduce(flat, ops)
        finally:
            if own:
                ctx.close()
    out, index = out.reshape(q.shape), index.reshape(q.shape[:-1])
    return (out, index) if return_index else out


def _window_offsets(window, nav_shape):
    """(k, 2) int32 (dy, dx) of the window's non-zero coefficients in C order, the origin left out."""
    from kikuchipy_amd.pattern._neighbours import dot_product_window, window_on_map

    win = dot_product_window(window, nav_shape)
    w = window_on_map(np.asarray(win) != 0, nav_shape) != 0
    wy, wx = w.shape
    off = [(j // wx - wy // 2, j % wx - wx // 2) for j in np.flatnonzero(w.ravel())]
    return np.array([o for o in off if o != (0, 0)], dtype=np.int32).reshape(-1, 2)


def _kam_host(q, ny, nx, ops, offsets, in_data, max_angle):
    one = sampling.rotation_group_operations("1")
    g = _normalise(q).reshape(ny, nx, 4)
    inside = np.ones((ny, nx), dtype=bool) if in_data is None else in_data.reshape(ny, nx)
    total, count = np.zeros((ny, nx)), np.zeros((ny, nx), dtype=np.int64)
    y, x = np.mgrid[0:ny, 0:nx]
    for dy, dx in offsets:
        yy, xx = y + dy, x + dx
        ok = (yy >= 0) & (yy < ny) & (xx >= 0) & (xx < nx)
        yc, xc = np.clip(yy, 0, ny - 1), np.clip(xx, 0, nx - 1)
        ok &= inside[yc, xc]
        w = _pair_angles_host(g.reshape(-1, 4), g[yc, xc].reshape(-1, 4), one, ops).reshape(ny, nx)
        if max_angle is not None:
            with np.errstate(invalid="ignore"):
                ok &= ~(w > max_angle)
        total = np.where(ok, total + w, total)
        count += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(count > 0, total / np.where(count > 0, count, 1), np.nan)
    return np.where(inside, out, np.nan)


def kernel_average_misorientation_map(rotations, point_group, nav_shape=None, window=None, max_angle=None,
                                      is_in_data=None, degrees=False, *, device=None, context=None):
    """The kernel average misorientation map: per map point the mean disorientation angle (float64, radians or
    `degrees`) to its neighbours under `window` - a `filters.Window` or a boolean array laid on the map as
    `get_average_neighbour_dot_product_map` lays its window (None: the nearest neighbours), the origin excluded.  Left
    out of the mean are neighbours outside the map, neighbours where `is_in_data` is false, and neighbours further than
    `max_angle` (in the unit `degrees` selects).  A point with no neighbour left, or not in the data, gives NaN.
    `nav_shape` is the map's shape (1 or 2 axes); None takes the leading axes of `rotations`."""
    q = _quaternions(rotations)
    nav = tuple(int(v) for v in (q.shape[:-1] if nav_shape is None else np.atleast_1d(nav_shape)))
    if not 1 <= len(nav) <= 2:
        raise ValueError("The map must have one or two navigation axes")
    flat = q.reshape(-1, 4)
    if flat.shape[0] != int(np.prod(nav)) or flat.shape[0] == 0:
        raise ValueError(f"{flat.shape[0]} rotations for a map of shape {nav}")
    ny, nx = (nav[0], 1) if len(nav) == 1 else nav
    ops = sampling.rotation_group_operations(sampling.rotation_group_name(point_group))
    offsets = _window_offsets(window, nav)
    mask = None
    if is_in_data is not None:
        mask = np.asarray(is_in_data, dtype=bool).reshape(-1)
        if mask.size != flat.shape[0]:
            raise ValueError(f"is_in_data of {mask.size} points for a map of shape {nav}")
    limit = None
    if max_angle is not None:
        limit = float(np.deg2rad(max_angle)) if degrees else float(max_angle)
        if not limit >= 0:
            raise ValueError(f"max_angle {max_angle}: zero or more")
    ctx, own = _context(device, context)
    if ctx is None:
        return _scale(_kam_host(flat, ny, nx, ops, offsets, mask, limit), degrees).reshape(nav)
    try:
        return ctx.orientation_kam(flat, ny, nx, ops, offsets, mask, limit, degrees).reshape(nav)
    finally:
        if own:
            ctx.close()
