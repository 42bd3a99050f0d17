"""The part of `kikuchipy.detectors.EBSDDetector` that dictionary generation reads
(detectors/_ebsd_detector.py of the reference): detector shape, one projection
centre (PC) and the sample/detector tilts -> gnomonic bounds and the
sample-to-detector orientation matrix that
`_get_direction_cosines_for_fixed_pc` takes
(signals/util/_master_pattern.py:83-124).

One PC, or one PC per map point (`pc` of shape navigation shape + (3,)):
dictionary generation uses a single PC for the whole dictionary (SURVEY.md
8(f1)), refinement takes either (8(f2)).  `get_indexer` returns the indexer of
Hough indexing.  Calibration from a grid of PCs -
`estimate_xtilt`, `estimate_xtilt_ztilt`, `fit_pc`, `extrapolate_pc` - and the
PC in the other vendors' conventions (`pc_emsoft`, `pc_bruker`, `pc_tsl`,
`pc_oxford`) are host NumPy (kikuchipy_amd/_pc_fit.py).
Plotting and file I/O are out of scope: `plot` and `figure_kwargs` are accepted
and nothing is drawn.
"""

import warnings

from collections.abc import Iterable
from numbers import Number

import numpy as np

# detectors/_ebsd_detector.py:71-91
PC_CONVENTIONS_ALIASES = {
    "bruker": ["bruker"],
    "tsl": ["tsl", "edax", "amatek"],
    "oxford": ["oxford", "aztec"],
    "emsoft": ["emsoft", "emsoft4", "emsoft5"],
}


def sample_to_detector_matrix(sample_tilt, tilt, azimuthal, twist):
    """Passive sample -> detector rotation matrix for angles in degrees
    (detectors/_ebsd_detector.py:100-150, :836-845).  Rows are the detector axes
    (X_d, Y_d, Z_d) in sample coordinates: start from (Y_s, Z_s, X_s) and turn
    all three about X_d by -sample_tilt, about X_d by +tilt, about Y_d by
    -azimuthal and about Z_d by -twist (axis-angle formula)."""
    basis = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], dtype=np.float64)
    angles = np.deg2rad(np.array([-sample_tilt, tilt, -azimuthal, -twist], dtype=np.float64))
    for axis_row, angle in zip((0, 0, 1, 2), angles):
        u = basis[axis_row] / np.sqrt(np.sum(np.square(basis[axis_row])))
        c, s = np.cos(angle), np.sin(angle)
        for j in range(3):
            v = basis[j].copy()
            basis[j] = v * c + np.cross(u, v) * s + u * np.dot(u, v) * (1.0 - c)
    return basis


class EBSDDetector:
    """EBSD detector with one projection centre, or one per map point.

    Parameters mirror the reference's constructor
    (detectors/_ebsd_detector.py:282-318): `shape` = (rows, columns), `px_size`
    in um, `binning`, detector `tilt`, `azimuthal` and `twist` and `sample_tilt`
    in degrees, `pc` = (PCx, PCy, PCz) in the given `convention` (stored in
    Bruker's convention like the reference does)."""

    def __init__(self, shape=(1, 1), px_size=1.0, binning=1, tilt=0.0, azimuthal=0.0, twist=0.0,
                 sample_tilt=70.0, pc=(0.5, 0.5, 0.5), convention="bruker"):
        self.shape = shape
        self.px_size = px_size
        self.binning = binning
        self.tilt = tilt
        self.azimuthal = azimuthal
        self.twist = twist
        self.sample_tilt = sample_tilt
        pc = np.atleast_2d(np.asarray(pc, dtype=np.float64))
        if pc.shape[-1] != 3 or pc.ndim > 3:
            raise ValueError(
                "`pc` must be (PCx, PCy, PCz) or an array of such triplets with at most two "
                f"navigation axes, got shape {pc.shape}"
            )
        self._pc = self._to_bruker(pc, convention)

    # detectors/_ebsd_detector.py:2207-2248, :2295-2315
    def _to_bruker(self, pc, convention):
        conv = None
        for name, aliases in PC_CONVENTIONS_ALIASES.items():
            if isinstance(convention, str) and convention.lower() in aliases:
                conv = name
        if conv is None:
            options = ", ".join(a for v in PC_CONVENTIONS_ALIASES.values() for a in v)
            raise ValueError(
                f"Invalid projection/pattern center convention {convention!r}. Options are {options}."
            )
        pcx, pcy, pcz = pc[..., 0], pc[..., 1], pc[..., 2]
        if conv == "tsl":
            return np.stack([pcx, 1 - pcy, pcz * min(self.nrows, self.ncols) / self.nrows], axis=-1)
        if conv == "oxford":
            return np.stack([pcx, 1 - pcy * self.aspect_ratio, pcz * self.aspect_ratio], axis=-1)
        if conv == "emsoft":
            version = int(convention[-1]) if convention[-1].isdigit() else 5
            if version < 5:
                pcx = -pcx
            return np.stack([
                0.5 - (pcx / (self.ncols * self._binning)),
                0.5 - (pcy / (self.nrows * self._binning)),
                pcz / (self.nrows * self._binning * self.px_size),
            ], axis=-1)
        return pc.copy()

    # ---- shape (detectors/_ebsd_detector.py:640-668)
    @property
    def nrows(self):
        return self.shape[0]

    @property
    def ncols(self):
        return self.shape[1]

    @property
    def size(self):
        return self.nrows * self.ncols

    @property
    def aspect_ratio(self):
        return self.ncols / self.nrows

    # ---- validated attributes: the reference's checks and texts (detectors/_ebsd_detector.py:2281-2292 and the setters
    # :337-340, :365-368, :392-395, :417-420, :582-585, :691-694)
    @property
    def shape(self):
        return self._shape

    @shape.setter
    def shape(self, value):
        if (not isinstance(value, Iterable) or isinstance(value, (str, bytes)) or len(value) != 2
                or not all(isinstance(v, Number) for v in value) or min(value) < 1):
            raise ValueError(f"Invalid shape {value}. Must be an iterable of two integers.")
        self._shape = tuple(int(v) for v in value)

    @property
    def binning(self):
        return int(self._binning)

    @binning.setter
    def binning(self, value):
        if not isinstance(value, Number):
            raise ValueError(f"Invalid binning {value}. Must be an integer.")
        self._binning = float(value)

    @property
    def px_size(self):
        return self._px_size

    @px_size.setter
    def px_size(self, value):
        if not isinstance(value, Number):
            raise ValueError(f"Invalid pixel size {value}. Must be a number.")
        self._px_size = float(value)

    def _angle(name, text):  # noqa: N805 - a small property factory
        def get(self):
            return getattr(self, "_" + name)

        def set_(self, value):
            if not isinstance(value, Number):
                raise ValueError(f"Invalid {text} {value!r}. Must be a number.")
            setattr(self, "_" + name, float(value))

        return property(get, set_)

    tilt = _angle("tilt", "detector tilt")
    azimuthal = _angle("azimuthal", "azimuthal")
    twist = _angle("twist", "twist")
    sample_tilt = _angle("sample_tilt", "sample tilt")
    del _angle

    @property
    def navigation_shape(self):
        return self._pc.shape[:-1]

    @property
    def navigation_size(self):
        return int(np.prod(self.navigation_shape))

    # ---- PC (Bruker convention); scalars for a single PC, arrays otherwise
    @property
    def pc(self):
        return self._pc

    @pc.setter
    def pc(self, value):
        value = np.atleast_2d(np.asarray(value, dtype=np.float64))
        if value.shape[-1] != 3:
            raise ValueError("`pc` must have a last axis of size 3")
        self._pc = value

    @property
    def pc_flattened(self):
        return self._pc.reshape(-1, 3)

    @property
    def pc_average(self):
        return np.nanmean(self.pc_flattened, axis=0)

    def _component(self, i):
        v = self._pc[..., i]
        return v[0] if v.shape == (1,) else v

    def _set_component(self, i, value):
        v = np.asarray(value, dtype=np.float64)
        if v.size > 1 and v.size == self.navigation_size:
            v = v.reshape(self._pc.shape[:-1])  # one value per projection centre, in any layout
        self._pc[..., i] = v

    @property
    def pcx(self):
        return self._component(0)

    @pcx.setter
    def pcx(self, value):
        self._set_component(0, value)

    @property
    def pcy(self):
        return self._component(1)

    @pcy.setter
    def pcy(self, value):
        self._set_component(1, value)

    @property
    def pcz(self):
        return self._component(2)

    @pcz.setter
    def pcz(self, value):
        self._set_component(2, value)

    # ---- derived sizes (detectors/_ebsd_detector.py:605-727)
    @property
    def navigation_dimension(self):
        return len(self.navigation_shape)

    @property
    def bounds(self):
        """Detector bounds [x0, x1, y0, y1] in pixel coordinates."""
        return np.array([0, self.ncols - 1, 0, self.nrows - 1])

    @property
    def unbinned_shape(self):
        return tuple(int(v) for v in np.array(self.shape, dtype=int) * self._binning)

    @property
    def height(self):
        """Detector height in microns."""
        return self.nrows * self.px_size * self._binning

    @property
    def width(self):
        """Detector width in microns."""
        return self.ncols * self.px_size * self._binning

    @property
    def px_size_binned(self):
        return self.px_size * self._binning

    @property
    def specimen_scintillator_distance(self):
        """PCz x detector height, in microns."""
        return self.pcz * self.height

    # ---- gnomonic coordinates (detectors/_ebsd_detector.py:731-818)
    @property
    def x_min(self):
        return -self.aspect_ratio * (self.pcx / self.pcz)

    @property
    def x_max(self):
        return self.aspect_ratio * (1 - self.pcx) / self.pcz

    @property
    def y_min(self):
        return -(1 - self.pcy) / self.pcz

    @property
    def y_max(self):
        return self.pcy / self.pcz

    @property
    def x_range(self):
        """(x_min, x_max) per projection centre: navigation shape + (2,)  (detectors/_ebsd_detector.py:749-755)."""
        return np.stack([np.atleast_1d(self.x_min), np.atleast_1d(self.x_max)], axis=-1).reshape(self.navigation_shape + (2,))

    @property
    def y_range(self):
        return np.stack([np.atleast_1d(self.y_min), np.atleast_1d(self.y_max)], axis=-1).reshape(self.navigation_shape + (2,))

    @property
    def x_scale(self):
        """Width of a pixel in gnomonic coordinates (detectors/_ebsd_detector.py:785-795)."""
        d = np.diff(self.x_range)
        return (d if self.ncols == 1 else d / (self.ncols - 1)).reshape(self.navigation_shape)

    @property
    def y_scale(self):
        d = np.diff(self.y_range)
        return (d if self.nrows == 1 else d / (self.nrows - 1)).reshape(self.navigation_shape)

    @property
    def r_max(self):
        """Largest distance from the pattern centre to a detector corner in gnomonic coordinates, with the corners the
        reference takes (detectors/_ebsd_detector.py:821-833: its "lower left" repeats the upper left)."""
        x0, x1, y0, y1 = (np.atleast_1d(v) for v in (self.x_min, self.x_max, self.y_min, self.y_max))
        corners = np.stack([x0**2 + y0**2, x1**2 + y0**2, x1**2 + y1**2, x0**2 + y0**2], axis=-1)
        return np.atleast_2d(np.sqrt(corners.max(axis=-1)).reshape(self.navigation_shape))

    @property
    def gnomonic_bounds(self):
        """(x_min, x_max, y_min, y_max): shape (4,) for one PC, else navigation shape + (4,)."""
        return np.stack([self.x_min, self.x_max, self.y_min, self.y_max], axis=-1).astype(np.float64)

    # ---- orientation
    @property
    def sample_to_detector(self):
        """3 x 3 matrix (the reference returns the same rotation as an orix `Rotation`)."""
        return sample_to_detector_matrix(self.sample_tilt, self.tilt, self.azimuthal, self.twist)

    @property
    def detector_to_sample(self):
        """`(~detector.sample_to_detector).to_matrix()`: the transpose."""
        return np.ascontiguousarray(self.sample_to_detector.T)

    def get_indexer(self, phase_list, reflectors=None, **kwargs):
        """A `HoughIndexer` for `EBSD.hough_indexing` and `EBSD.hough_indexing_optimize_pc` from this detector's shape,
        PC(s), sample tilt and tilt (detectors/_ebsd_detector.py:1598 of the reference).  `phase_list`: a phase or a list
        of phases, each a `Reflectors`, a (`Reflectors` or hkl array, point group) pair, or a point-group name (a cubic
        lattice); `reflectors`: None, or per phase the hkl to index with.  `**kwargs` of the band detection: `nBands` (9),
        `nTheta` (180), `nRho`, `tSigma`, `rSigma`, `rhoMaskFrac`; anything else raises `TypeError`.  The algorithm is
        this package's own (kikuchipy_amd/indexing/_hough_indexing.py), not PyEBSDIndex's."""
        from kikuchipy_amd.indexing._hough_indexing import indexer_from_detector

        return indexer_from_detector(self, phase_list, reflectors, **kwargs)

    # ---- the PC in the vendors' conventions (detectors/_ebsd_detector.py:1660-1775, :2317-2336): the inverses of `_to_bruker`
    def pc_emsoft(self, version=5):
        """The PC(s) in EMsoft's convention (xpc, ypc, L): xpc = Nx b (1 / 2 - PCx), ypc = Ny b (1 / 2 - PCy),
        L = Ny b px_size PCz; xpc changes sign before `version` 5."""
        new_pc = np.zeros_like(self.pc, dtype=float)
        new_pc[..., 0] = (0.5 - self.pcx) * self.ncols * self._binning
        if version < 5:
            new_pc[..., 0] = -new_pc[..., 0]
        new_pc[..., 1] = (0.5 - self.pcy) * self.nrows * self._binning
        new_pc[..., 2] = self.pcz * self.nrows * self._binning * self.px_size
        return new_pc

    def pc_bruker(self):
        """The PC(s) in Bruker's convention, the one they are stored in."""
        return self.pc

    def pc_tsl(self):
        """The PC(s) in EDAX TSL's convention: (PCx, 1 - PCy, PCz Ny / min(Ny, Nx))."""
        new_pc = self.pc.copy()
        new_pc[..., 1] = 1 - self.pcy
        new_pc[..., 2] /= min([self.nrows, self.ncols]) / self.nrows
        return new_pc

    def pc_oxford(self):
        """The PC(s) in Oxford Instruments' convention: (PCx, (1 - PCy) / aspect ratio, PCz / aspect ratio)."""
        new_pc = self.pc.copy()
        new_pc[..., 1] = (1 - self.pcy) / self.aspect_ratio
        new_pc[..., 2] /= self.aspect_ratio
        return new_pc

    # ---- calibration from a grid of PCs (detectors/_ebsd_detector.py:1045-1596; _fit_projection_center.py)
    def _warn_if_angles_ignored(self, msg):
        if self.azimuthal != 0.0 or self.twist != 0.0:
            warnings.warn(msg + f" azimuthal={self.azimuthal} and twist={self.twist} will be ignored.", UserWarning, stacklevel=3)

    @staticmethod
    def _no_figure(name):
        raise NotImplementedError(f"`{name}(return_figure=True)` needs Matplotlib, which this package does not use: plot the "
                                  "PCs of the returned detector")

    def estimate_xtilt(self, detect_outliers=False, plot=True, degrees=False, return_figure=False, return_outliers=False,
                       figure_kwargs=None):
        """An estimate of the tilt about the detector X_d axis that brings the sample normal onto the detector normal:
        pi / 2 + atan(slope) of the straight line PCy(PCz) through the PCs - ordinary least squares with an intercept,
        or with `detect_outliers` (which `return_outliers` implies) a robust fit that also names the outliers, returned
        as a mask of the navigation shape.  Radians unless `degrees`.

        The reference's robust fit is scikit-learn's `RANSACRegressor` with its random trials.  scikit-learn is not
        available to this package, so the robust fit is this package's own and deterministic: scikit-learn's rules and
        defaults - a model through two PCs, the median absolute deviation of PCy as the residual threshold - over ALL
        pairs of PCs in lexicographic order; most inliers win, then the higher R^2 on the inliers, then the first
        pair; the line is fitted again to the inliers (kikuchipy_amd/_pc_fit.py).  Where the outliers stand clear of the
        threshold the two name the same PCs; its numbers are NOT scikit-learn's otherwise.

        `plot` and `figure_kwargs` are accepted and nothing is drawn; `return_figure` is refused."""
        from kikuchipy_amd import _pc_fit

        if self.navigation_size == 1:
            raise ValueError("Estimation requires more than one projection center")
        if return_figure:
            self._no_figure("estimate_xtilt")
        self._warn_if_angles_ignored("estimate_xtilt() assumes azimuthal and twist angles are zero, but")
        if return_outliers:
            detect_outliers = True
        pcy, pcz = self.pcy.reshape(-1), self.pcz.reshape(-1)
        if detect_outliers:
            slope, _, is_inlier = _pc_fit.robust_linear_fit(pcz, pcy)
            is_outlier = ~is_inlier
        else:
            slope, _ = _pc_fit.linear_fit(pcz, pcy)
            is_outlier = None
        x_tilt = float(np.pi / 2 + np.arctan(slope))
        out = (float(np.rad2deg(x_tilt)),) if degrees else (x_tilt,)
        if is_outlier is not None:
            out += (is_outlier.reshape(self.navigation_shape),)
        return out[0] if len(out) == 1 else out

    def estimate_xtilt_ztilt(self, degrees=False, is_outlier=None):
        """Estimates of the tilts about the detector X_d and Z_d axes that bring the sample normal onto the detector
        normal, from a plane fitted to the PCs (those not `is_outlier`, a mask of the navigation shape) by a singular
        value decomposition about their 10 % trimmed mean."""
        from kikuchipy_amd import _pc_fit

        if self.navigation_size == 1:
            raise ValueError("Estimation requires more than one projection center")
        self._warn_if_angles_ignored("estimate_xtilt_ztilt() assumes azimuthal and twist angles are zero, but")
        pc = self.pc
        if isinstance(is_outlier, np.ndarray):
            pc = pc[~is_outlier]
        pc = pc.reshape((-1, 3))
        x_tilt, z_tilt, *_ = _pc_fit.fit_hyperplane(pc - pc.mean(axis=0))
        if degrees:
            x_tilt, z_tilt = np.rad2deg(x_tilt), np.rad2deg(z_tilt)
        return x_tilt, z_tilt

    def extrapolate_pc(self, pc_indices, navigation_shape, step_sizes, shape=None, px_size=None, binning=None, is_outlier=None):
        """A new detector with a PC for every point of a map of `navigation_shape`, extrapolated from the average of
        this detector's PCs (those not `is_outlier`), taken to belong to the rounded average of `pc_indices` - (row,
        column) of each PC, shape (2,) + the number of PCs, possibly outside the map:
        PCx = mean PCx + (mean column - column) dx / (px_size binning Nx),
        PCy = mean PCy + (mean row - row) dy cos(alpha) / (px_size binning Ny),
        PCz = mean PCz - (mean row - row) dy sin(alpha) / (px_size binning Ny), alpha = 90 - sample tilt + detector tilt
        in degrees, (dy, dx) = `step_sizes`; `shape`, `px_size` and `binning` default to the detector's and are those of
        the new detector.  (The average position is taken exactly as the reference takes it: the indices are
        transposed to one row per PC and averaged along the second axis.)"""
        dy, dx = step_sizes
        pc_indices = np.atleast_2d(pc_indices).T
        ny, nx = navigation_shape
        if shape is None:
            shape = self.shape
        nrows, ncols = shape
        if px_size is None:
            px_size = self.px_size
        if binning is None:
            binning = float(self.binning)
        pc = self.pc_flattened
        if is_outlier is not None:
            is_inlier = ~np.asarray(is_outlier)
            pc = pc[is_inlier]
            pc_indices = pc_indices[is_inlier]
        pc_mean = pc.mean(axis=0)
        pc_indices_mean = np.round(pc_indices.mean(axis=1)).astype(int)
        self._warn_if_angles_ignored("extrapolate_pc() assumes azimuthal and twist angles are zero, but")
        alpha = np.deg2rad(90 - self.sample_tilt + self.tilt)
        y, x = np.indices((ny, nx), dtype=float)
        factor = px_size * binning
        d_pcx = -(pc_indices_mean[1] - x) * dx / (factor * ncols)
        d_pcy = -(pc_indices_mean[0] - y) * dy * np.cos(alpha) / (factor * nrows)
        d_pcz = +(pc_indices_mean[0] - y) * dy * np.sin(alpha) / (factor * nrows)
        new_detector = self.deepcopy()
        new_detector.shape = shape
        new_detector.pc = np.stack((pc_mean[0] - d_pcx, pc_mean[1] - d_pcy, pc_mean[2] - d_pcz), axis=2)
        new_detector.px_size = px_size
        new_detector.binning = int(binning)
        return new_detector

    def fit_pc(self, pc_indices, map_indices, transformation="projective", is_outlier=None, plot=True, return_figure=False,
               figure_kwargs=None):
        """A new detector with a PC for every map point of `map_indices` - (2, m) or (2, n, m) rows and columns - from a
        plane fitted to this detector's PCs at `pc_indices`, (2,) + the navigation shape, leaving out those `is_outlier`.
        "affine": a least-squares affine map from (row, column, 1) to the PC.  "projective" (default): the PCs are turned
        into their fitted plane (`estimate_xtilt_ztilt`'s), a homography from the indices to the in-plane coordinates is
        estimated by the normalised direct linear transformation, and the projected indices are turned back.  The new
        detector's `sample_tilt` is 90 - x tilt - detector tilt, the x tilt from the straight line through the fitted
        (PCz, PCy).  `plot` and `figure_kwargs` are accepted and nothing is drawn; `return_figure` is refused."""
        from kikuchipy_amd import _pc_fit

        n_pc = self.navigation_size
        if n_pc == 1:
            raise ValueError("Fitting requires multiple projection centers (PCs)")
        if return_figure:
            self._no_figure("fit_pc")
        pc_indices, map_indices = np.asarray(pc_indices), np.asarray(map_indices)
        nav_shape = self.navigation_shape
        if pc_indices.shape != (2,) + nav_shape:
            raise ValueError(f"`pc_indices` array shape {pc_indices.shape} must be equal to {(2,) + nav_shape}")
        if map_indices.ndim not in [2, 3] or map_indices.shape[0] != 2:
            raise ValueError(f"`map_indices` array shape {map_indices.shape} must be (2, m columns) or (2, n rows, m columns)")
        if is_outlier is not None and (not isinstance(is_outlier, np.ndarray) or not np.issubdtype(is_outlier.dtype, np.bool_)
                                       or is_outlier.size != n_pc):
            raise ValueError("`is_outlier` must be a boolean array of a size equal to the number of PCs")
        _, pc_fit_map, _, x_tilt, _, _ = _pc_fit.fit_plane_to_pc(self.pc_flattened, pc_indices, map_indices, is_outlier,
                                                                 transformation)
        new_detector = self.deepcopy()
        new_detector.pc = pc_fit_map
        self._warn_if_angles_ignored("fit_pc() assumes azimuthal and twist angles are zero when estimating sample_tilt, but")
        new_detector.sample_tilt = float(90 - np.rad2deg(x_tilt) - new_detector.tilt)
        return new_detector

    def crop(self, extent):
        """A new detector cropped to `extent` = (top, bottom, left, right) in pixels, its PC values updated
        (detectors/_ebsd_detector.py:986-1032): the extent is clamped to the detector; it must be integers with
        bottom > top and right > left after that.  (The reference builds the new detector without `twist`; here it is
        carried over like the other angles.)"""
        refusal = "Extent (top, bottom, left, right) must be integers and given so that bottom > top and right > left"
        # one pass over the two axes: (first, end) of the extent on an axis of `size` pixels, cut to [0, size]
        kept = []
        for size, (first, end) in zip(self.shape, (extent[0:2], extent[2:4])):
            if len(extent) != 4 or not (isinstance(first, int) and isinstance(end, int)):
                raise ValueError(refusal)
            first, end = (0 if first < 0 else first), (size if end > size else end)
            if end <= first:
                raise ValueError(refusal)
            kept.append((first, end - first))
        (top, rows), (left, cols) = kept
        ny, nx = self.shape
        pc = np.stack([(self._pc[..., 0] * nx - left) / cols,
                       (self._pc[..., 1] * ny - top) / rows,
                       self._pc[..., 2] * ny / rows], axis=-1)
        return EBSDDetector((rows, cols), self.px_size, self._binning, self.tilt, self.azimuthal, self.twist,
                            self.sample_tilt, pc, "bruker")

    def deepcopy(self):
        return EBSDDetector(self.shape, self.px_size, self._binning, self.tilt, self.azimuthal, self.twist,
                            self.sample_tilt, self._pc.copy(), "bruker")

    def __repr__(self):
        """The reference's text (detectors/_ebsd_detector.py:319-331)."""
        pc = tuple(float(v) for v in np.round(self.pc_average, 3))
        deg = "\N{DEGREE SIGN}"
        return ("EBSDDetector\n"
                f"  shape (Ny, Nx):     {self.shape}\n"
                f"  pc (PCx, PCy, PCz): {pc}\n"
                f"  sample_tilt:        {self.sample_tilt}{deg}\n"
                f"  tilt:               {self.tilt}{deg}\n"
                f"  azimuthal:          {self.azimuthal}{deg}\n"
                f"  twist:              {self.twist}{deg}\n"
                f"  binning:            {self.binning}\n"
                f"  px_size:            {self.px_size} um")
