"""NumPy restatement of virtual BSE imaging (imaging/vbse.py, signals/ebsd.py:1555-1598 and :3091-3105) for the host and
GPU tests: the ROI -> slice rule, `nansum` over the two signal axes, the loops of `get_images_from_grid` /
`get_rgb_image` and the channel arithmetic of `_get_rgb_image`.  tools/gen_vbse_golden.py asserts that `rgb` here gives
the bytes of the reference's own `_get_rgb_image` for every case of the fixture; the slice rule is restated from memory
of HyperSpy (not importable here) and is pinned by the reference's tests for whole-pixel edges only."""

import numpy as np


def index(value, size, scale=1.0, offset=0.0, default=0):
    """Axis value -> index: below the axis 0, beyond the last pixel's coordinate `size`, else round half to even."""
    if value is None:
        return default
    if value < offset:
        return 0
    if value > offset + (size - 1) * scale:
        return size
    return int(round((value - offset) / scale))


def roi_rect(left, top, right, bottom, shape):
    sy, sx = shape
    c0, c1 = index(left, sx), index(right, sx, default=sx)
    r0, r1 = index(top, sy), index(bottom, sy, default=sy)
    return r0, max(r0, r1), c0, max(c0, c1)


def grid_edges(shape, grid):
    return np.linspace(0, shape[0], grid[0] + 1, dtype=np.float64), np.linspace(0, shape[1], grid[1] + 1, dtype=np.float64)


def tile_roi(shape, grid, index_):
    """(left, top, right, bottom) of `roi_from_grid` (vbse.py:303-318) for one tile (row, col) or a list of tiles."""
    rows, cols = grid_edges(shape, grid)
    idx = np.array([index_] if isinstance(index_, tuple) else index_)
    return (cols[min(idx[:, 1])], rows[min(idx[:, 0])], cols[max(idx[:, 1])] + cols[1], rows[max(idx[:, 0])] + rows[1])


def tile_rect(shape, grid, index_):
    return roi_rect(*tile_roi(shape, grid, index_), shape)


def grid_rects(shape, grid):
    return [tile_rect(shape, grid, (r, c)) for r, c in np.ndindex(*grid)]


def region_sum(data, rect):
    """`roi(signal).nansum(signal_axes)`: NumPy's own sum (uint64 / int64 for integers, pairwise in the data's dtype for
    floats)."""
    r0, r1, c0, c1 = rect
    return np.nansum(data[..., r0:r1, c0:c1], axis=(-2, -1))


def region_sums(data, rects):
    if not len(rects):
        return np.zeros(data.shape[:-2] + (0,), dtype=np.nansum(data[..., :0, :0], axis=(-2, -1)).dtype)
    return np.stack([region_sum(data, r) for r in rects], axis=-1)


def region_sums_f64(data, rects):
    """(sum, sum |x|, number of pixels) per region in float64, NaN as 0: the centre and the scale of the float bound."""
    x = np.nan_to_num(np.asarray(data, dtype=np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf)
    s = np.stack([x[..., r0:r1, c0:c1].sum(axis=(-2, -1)) for r0, r1, c0, c1 in rects], axis=-1)
    a = np.stack([np.abs(x[..., r0:r1, c0:c1]).sum(axis=(-2, -1)) for r0, r1, c0, c1 in rects], axis=-1)
    n = np.array([(r1 - r0) * (c1 - c0) for r0, r1, c0, c1 in rects])
    return s, a, n


def images_from_grid(data, grid, dtype_out="float32"):
    shape = data.shape[-2:]
    images = np.zeros(tuple(grid) + data.shape[:-2], dtype=np.dtype(dtype_out))
    for row, col in np.ndindex(*grid):
        images[row, col] = region_sum(data, tile_rect(shape, grid, (row, col)))
    return images


def channel_rects(shape, grid, rois):
    """The rectangles of one channel: a grid index tuple, a (left, top, right, bottom) list-ROI `("roi", l, t, r, b)`,
    or a list of either."""
    if isinstance(rois, tuple):
        rois = [rois]
    out = []
    for roi in rois:
        if len(roi) == 5 and roi[0] == "roi":
            out.append(roi_rect(*roi[1:], shape))
        else:
            out.append(tile_rect(shape, grid, roi))
    return out


def channels(data, grid, r, g, b, sums=region_sum):
    shape = data.shape[-2:]
    out = []
    for rois in (r, g, b):
        image = np.zeros(data.shape[:-2], dtype=np.float64)
        for rect in channel_rects(shape, grid, rois):
            image += sums(data, rect)
        out.append(image)
    return out


def rgb(chans, percentiles=None, normalize=True, alpha=None, dtype_out="uint8", add_bright=0, contrast=1.0):
    """vbse.py:458-524 with `_normalize_image` (:416-455) and `rescale_intensity` (pattern/_pattern.py:31-111) written
    out; float32 throughout except the alpha factor, which is float64 and multiplied into the float32 image in place."""
    dt = np.dtype(dtype_out)
    top = int(np.iinfo(dt).max)
    img = np.zeros(chans[0].shape + (3,), np.float32)
    for i, ch in enumerate(chans):
        if normalize:
            ch = ch.astype(np.float32)
            gain = contrast * (top * 0.3125)
            ch = np.clip((top // 2 + add_bright) + ((gain * (ch - np.median(ch))) / np.std(ch)), 0, top)
        img[..., i] = ch
    if alpha is not None:
        lo = np.nanmin(alpha)
        factor = (alpha - lo) / (np.nanmax(alpha) - lo)
        for i in range(3):
            img[..., i] *= factor
    if percentiles is not None:
        lo, hi = tuple(np.percentile(img, q=percentiles))
        img = np.clip(img, lo, hi)
    else:
        lo, hi = np.nanmin(img), np.nanmax(img)
    return (((img - lo) / float(hi - lo)) * (top - 0) + 0).astype(dt)
