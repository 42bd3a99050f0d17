"""Virtual backscatter electron (BSE) imaging on the GPU (imaging/vbse.py, signals/ebsd.py:1555-1598).

`VirtualBSEImager` forms images of a map from the intensity within rectangles on the detector: all tiles of a grid, or
three (lists of) rectangles as the red, green and blue channel.  Whatever the number of rectangles, their sums over
every pattern come from ONE pass over the patterns on the device (`kikuchipy_amd.pattern.region_sums`,
csrc/regionsum.hip); what follows touches a few numbers per map point and runs on the host in the reference's NumPy
arithmetic.  A region of interest (ROI) is anything with `left`, `top`, `right`, `bottom` (HyperSpy's
`RectangularROI` too); `roi_to_rect` alone turns one into pixel indices.  `plot_grid` has no counterpart: the package
does not plot.
"""

import numpy as np

from kikuchipy_amd.pattern import _pattern
from kikuchipy_amd.signals import VirtualBSEImage


class RectangularROI:
    """Stand-in for `hyperspy.roi.RectangularROI`: a rectangle in the coordinates of the signal axes (x to the right,
    y down), `None` for a side that is open."""

    def __init__(self, left=None, top=None, right=None, bottom=None):
        self.left, self.top, self.right, self.bottom = left, top, right, bottom

    def __repr__(self):
        return f"RectangularROI(left={self.left:g}, top={self.top:g}, right={self.right:g}, bottom={self.bottom:g})"


def signal_axes(signal):
    """((x scale, x offset), (y scale, y offset)) of the signal axes: from `signal.axes_manager.signal_axes`
    (HyperSpy's order, x first) where the signal has them, else 1 and 0."""
    axes = getattr(getattr(signal, "axes_manager", None), "signal_axes", None)
    if axes is None or len(axes) != 2:
        return (1.0, 0.0), (1.0, 0.0)
    return tuple((float(a.scale), float(getattr(a, "offset", 0.0))) for a in axes)


def _index(value, size, scale, offset, default):
    if value is None:
        return default
    if value < offset:  # below the axis
        return 0
    if value > offset + (size - 1) * scale:  # beyond the last pixel's coordinate
        return size
    return int(round((value - offset) / scale))


def roi_to_rect(roi, signal_shape, axes=((1.0, 0.0), (1.0, 0.0))):
    """The pixels (row0, row1, col0, col1), half-open, that `roi` selects on a detector of `signal_shape` (sy, sx) with
    the axes (`signal_axes`).  THE one place that holds the rule, written after HyperSpy's `value2index` and
    `RectangularROI._make_slices` (HyperSpy is not a dependency and was not at hand to compare): a side at `value` is
    the index `round((value - offset) / scale)` with Python's round (halves go to the even index); a value below the
    axis is index 0, one beyond the coordinate of the last pixel is `size` - so `right=60` on 60 pixels selects up to
    the end.  The reference's tests pin this only for sides at whole pixels.  Anything without `left`, `top`, `right`
    and `bottom` (circles, lines) raises NotImplementedError."""
    if not all(hasattr(roi, a) for a in ("left", "top", "right", "bottom")):
        raise NotImplementedError(f"{type(roi).__name__}: only rectangular ROIs (left, top, right, bottom) are supported")
    sy, sx = (int(v) for v in signal_shape)
    (dx, ox), (dy, oy) = axes
    col0, col1 = _index(roi.left, sx, dx, ox, 0), _index(roi.right, sx, dx, ox, sx)
    row0, row1 = _index(roi.top, sy, dy, oy, 0), _index(roi.bottom, sy, dy, oy, sy)
    return row0, max(row0, row1), col0, max(col0, col1)


class VirtualBSEImager:
    """imaging/vbse.py:31-318 for an `EBSD` signal of this package."""

    def __init__(self, signal):
        self._signal = signal
        self.grid_shape = tuple(min(5, size) for size in signal._signal_shape_rc)

    @property
    def signal(self):
        return self._signal

    @property
    def grid_shape(self):
        """(rows, columns) of the detector grid; at most the signal shape."""
        return self._grid_shape

    @grid_shape.setter
    def grid_shape(self, shape):
        sig = self._signal._signal_shape_rc
        if len(shape) != len(sig):
            raise ValueError(f"Grid shape must have the same length as number of signal dimensions {len(sig)}")
        if any(i > j for i, j in zip(shape, sig)):
            raise ValueError(f"Grid shape (n rows, n cols) = {shape} cannot be greater than signal shape {sig}")
        self._grid_shape = shape

    @property
    def grid_rows(self):
        return np.linspace(0, self._signal._signal_shape_rc[0], self.grid_shape[0] + 1, dtype=np.float64)

    @property
    def grid_cols(self):
        return np.linspace(0, self._signal._signal_shape_rc[1], self.grid_shape[1] + 1, dtype=np.float64)

    def __repr__(self):
        return f"{self.__class__.__name__} for " + repr(self._signal)

    def roi_from_grid(self, index):
        """The ROI of one grid tile (row, column), or the one spanning a list of tiles; the far edges are
        `rows[max] + rows[1]` as in the reference (vbse.py:311-314), not `rows[max + 1]`."""
        rows, cols = self.grid_rows, self.grid_cols
        (dc, _), (dr, _) = signal_axes(self._signal)
        if isinstance(index, tuple):
            index = [index]
        index = np.array(index)
        return RectangularROI(left=cols[min(index[:, 1])] * dc, top=rows[min(index[:, 0])] * dr,
                              right=(cols[max(index[:, 1])] + cols[1]) * dc, bottom=(rows[max(index[:, 0])] + rows[1]) * dr)

    def _rect(self, roi):
        if isinstance(roi, tuple):
            roi = self.roi_from_grid(roi)
        return roi_to_rect(roi, self._signal._signal_shape_rc, signal_axes(self._signal))

    def get_images_from_grid(self, dtype_out="float32", *, devices=None):
        """vbse.py:239-283: the image of every grid tile, `grid_shape` + navigation shape of `dtype_out` (cast as NumPy's
        assignment does), from one pass over the patterns."""
        dtype_out = np.dtype(dtype_out)
        grid = tuple(self.grid_shape)
        rects = [self._rect((row, col)) for row, col in np.ndindex(*grid)]
        sums = self._signal._region_sums(rects, devices)
        images = np.zeros(grid + self._signal._navigation_shape_rc, dtype=dtype_out)
        images[...] = np.moveaxis(sums, -1, 0).reshape(images.shape)
        return VirtualBSEImage(images)

    def get_rgb_image(self, r, g, b, percentiles=None, normalize=True, alpha=None, dtype_out="uint8", add_bright=0,
                      contrast=1.0, *, devices=None):
        """vbse.py:135-237: an RGB image (ny, nx, 3) of `dtype_out` (uint8 or uint16; `.rgb_data` is HyperSpy's
        rgb8 / rgb16 view).  A channel is a ROI, a grid index (row, column) or a list of either, and is the float64 sum
        of their images; all rectangles of the three channels are summed in one pass over the patterns.  Then, as
        there: each channel normalized (`normalize`: median to mid-range, one standard deviation to 0.3125 of the range
        times `contrast`, plus `add_bright`, clipped), multiplied by `alpha` scaled to [0, 1], and the whole image
        rescaled to the range of `dtype_out`, between `percentiles` of it if given."""
        dtype_out = np.dtype(dtype_out)
        if dtype_out not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise ValueError(f"dtype_out must be uint8 or uint16, not {dtype_out}")
        nav = self._signal._navigation_shape_rc
        if len(nav) != 2:  # what HyperSpy answers to the reference when it makes the RGB signal of a 1-D map
            raise ValueError(f"The signal dimension cannot be greater than the number of axes which is {len(nav)}")
        rects, counts = [], []
        for rois in (r, g, b):
            if isinstance(rois, tuple) or not hasattr(rois, "__iter__"):
                rois = (rois,)
            rois = list(rois)
            rects += [self._rect(roi) for roi in rois]
            counts.append(len(rois))
        sums = self._signal._region_sums(rects, devices)
        channels, i = [], 0
        for n in counts:
            image = np.zeros(nav, dtype=np.float64)
            for _ in range(n):
                image += sums[..., i]
                i += 1
            channels.append(image)
        if isinstance(alpha, VirtualBSEImage):
            alpha = alpha.data
        rgb = rgb_image(channels, percentiles, normalize, alpha, dtype_out, add_bright, contrast)
        return VirtualBSEImage(rgb)


def normalize_image(image, add_bright=0, contrast=1.0, dtype_out="uint8"):
    """vbse.py:416-455: `offset + contrast * (image - median) / std` clipped to the range of `dtype_out`, with
    offset = max // 2 + add_bright and the contrast in units of 0.3125 max per standard deviation."""
    dtype_max = np.iinfo(np.dtype(dtype_out)).max
    offset = (dtype_max // 2) + add_bright
    contrast = contrast * (dtype_max * 0.3125)
    median = np.median(image)
    std = np.std(image)
    return np.clip(offset + ((contrast * (image - median)) / std), 0, dtype_max)


def rgb_image(channels, percentiles=None, normalize=True, alpha=None, dtype_out="uint8", add_bright=0, contrast=1.0):
    """vbse.py:458-524 and the `rescale_intensity` of pattern/_pattern.py:31-111 it ends in, operation by operation
    (float32 image, float64 alpha multiplied in place), so that the bytes are the reference's: three channels of the
    map's shape -> (ny, nx, 3) of `dtype_out`."""
    dtype_out = np.dtype(dtype_out)
    rgb = np.zeros(channels[0].shape + (3,), np.float32)
    for i, channel in enumerate(channels):
        if normalize:
            channel = normalize_image(channel.astype(np.float32), add_bright, contrast, dtype_out)
        rgb[..., i] = channel
    if alpha is not None:
        alpha_min = np.nanmin(alpha)
        rescaled_alpha = (alpha - alpha_min) / (np.nanmax(alpha) - alpha_min)
        for i in range(3):
            rgb[..., i] *= rescaled_alpha
    if percentiles is not None:
        imin, imax = tuple(np.percentile(rgb, q=percentiles))
        rgb = np.clip(rgb, imin, imax)
    else:
        imin, imax = np.nanmin(rgb), np.nanmax(rgb)
    omin, omax = _pattern.DTYPE_RANGE[dtype_out.type]
    rescaled = (rgb - imin) / float(imax - imin)
    return (rescaled * (omax - omin) + omin).astype(dtype_out)
