"""Dictionary generation: `EBSDMasterPattern.get_patterns`
(signals/ebsd_master_pattern.py:95-330 of the reference) on the GPU engine.

`ProjectedDictionary` is what `get_patterns(..., compute=False)` hands back in
place of the reference's Dask array: an (N, rows, cols) lazy array that knows
how its patterns are made (master pattern, detector, one rotation per
pattern).  `kikuchipy_amd.dictionary_indexing` recognises it and has the
engine generate every dictionary chunk directly in device memory
(`kpdi_push_rotations_chunk`), so the dictionary never crosses PCIe and is
never materialised on the host; `.compute()` materialises it (also on the
GPU) for any other use.

`KikuchiPatternSimulator.calculate_master_pattern`
(simulations/kikuchi_pattern_simulator.py:122-215 of the reference) makes a
dictionary source without EMsoft: the kinematical master pattern of a list of
reflectors in the stereographic projection, summed on the GPU
(csrc/kinematical.hip), which `EBSDMasterPattern.as_lambert` turns into the
projection that `get_patterns` reads.  `Reflectors` is the plain holder of the
reflector list (diffsims is not a dependency).

`KikuchiPatternSimulator.on_detector` (simulations/kikuchi_pattern_simulator.py:217-380 of the reference) projects the
Kikuchi lines and zone axes of every map point onto the detector on the GPU (csrc/geometrical.hip) and returns a
`GeometricalKikuchiPatternSimulation` (simulations/_kikuchi_pattern_simulation.py), whose `lines_coordinates` and
`zone_axes_coordinates` are what a plot is fed with; plotting itself is not part of this package.
"""

import copy

import numpy as np

from kikuchipy_amd import _lib

# skimage.util.dtype.dtype_range as used at signals/ebsd_master_pattern.py:226-227
DTYPE_RANGE = {
    np.dtype(np.float32): (-1.0, 1.0),
    np.dtype(np.float64): (-1.0, 1.0),
    np.dtype(np.uint8): (0.0, 255.0),
    np.dtype(np.uint16): (0.0, 65535.0),
}


class ProjectedDictionary:
    """Lazy (N, rows, cols) array of simulated patterns; quacks like the Dask
    array the reference returns as far as dictionary indexing reads it
    (`ndim`, `shape`, `dtype`, `chunksize`, slicing along axis 0, `compute()`)."""

    def __init__(self, master_upper, master_lower, rotations, detector, rescale, out_min, out_max,
                 dtype_out=np.float32, device=0, chunk=None, _root=None, pcs=None):
        """`pcs`: None - the detector's one projection centre for every pattern; (N, 3) - one PC per pattern (a detector
        with a PC for every rotation: signals/ebsd_master_pattern.py:236-241, :274-283 of the reference)."""
        self.master_upper = master_upper
        self.master_lower = master_lower
        self.rotations = np.ascontiguousarray(rotations, dtype=np.float64).reshape(-1, 4)
        self.pcs = None if pcs is None else np.ascontiguousarray(pcs, dtype=np.float64).reshape(-1, 3)
        if self.pcs is not None and self.pcs.shape[0] != self.rotations.shape[0]:
            raise ValueError(f"{self.rotations.shape[0]} rotations but {self.pcs.shape[0]} projection centres")
        self.detector = detector
        self.rescale = bool(rescale)
        self.out_min, self.out_max = float(out_min), float(out_max)
        self.dtype = np.dtype(dtype_out)
        if self.dtype not in DTYPE_RANGE:
            raise ValueError(f"dtype_out {self.dtype} is not supported (float32, float64, uint8, uint16)")
        self.device = device
        self._chunk = chunk
        self._root = _root if _root is not None else self  # slices share the root's context
        self._ctx = None

    # ---- array protocol
    @property
    def shape(self):
        return (self.rotations.shape[0],) + self.detector.shape

    ndim = 3

    @property
    def chunksize(self):
        n = self.rotations.shape[0]
        if self._chunk is None:
            # 8 GiB of float32 patterns per iteration: a chunk only ever exists in device memory
            # (raw + prepared = 16 of the 288 GiB), and fewer, larger sweeps waste less on launch tails
            per = max(1, (8 << 30) // (4 * self.detector.size))
            return (min(n, per),) + self.detector.shape
        return (min(n, self._chunk),) + self.detector.shape

    def __len__(self):
        return self.rotations.shape[0]

    def __getitem__(self, key):
        if isinstance(key, tuple):
            if len(key) != 1 and any(k != slice(None) for k in key[1:]):
                raise IndexError("a ProjectedDictionary can only be sliced along its first axis")
            key = key[0]
        if isinstance(key, (int, np.integer)):
            return self[key:key + 1 if key != -1 else None].compute()[0]
        if not isinstance(key, slice):
            raise IndexError("a ProjectedDictionary can only be sliced along its first axis")
        return ProjectedDictionary(self.master_upper, self.master_lower, self.rotations[key], self.detector,
                                   self.rescale, self.out_min, self.out_max, self.dtype, self.device,
                                   self._chunk, _root=self._root, pcs=None if self.pcs is None else self.pcs[key])

    # ---- engine
    def configure(self, ctx):
        """Make `ctx` hold this dictionary's master pattern and detector (once)."""
        # `Context.set_master_pattern / set_detector / set_direction_cosines` reset the key, so a
        # refinement on the same context (which loads ITS master pattern) cannot leave a stale match;
        # the detector enters by value: an in-place change of its PC must reach the engine
        det = self.detector
        if self.pcs is not None:  # one PC per pattern: the direction cosines are formed on the device, per pattern
            key = (id(self.master_upper), id(self.master_lower), "one PC per pattern")
            if getattr(ctx, "_projection_key", None) != key:
                ctx.set_master_pattern(self.master_upper, self.master_lower)
                ctx._projection_key = key
                ctx._projection_refs = (self.master_upper, self.master_lower, det)
            return
        key = (id(self.master_upper), id(self.master_lower), tuple(np.ravel(det.gnomonic_bounds)), float(det.pcz),
               det.nrows, det.ncols, tuple(np.ravel(det.detector_to_sample)))
        if getattr(ctx, "_projection_key", None) != key:
            ctx.set_master_pattern(self.master_upper, self.master_lower)
            ctx.set_detector(det.gnomonic_bounds, det.pcz, det.nrows, det.ncols, det.detector_to_sample)
            ctx._projection_key = key
            ctx._projection_refs = (self.master_upper, self.master_lower, det)  # keep the ids alive

    def push_to_engine(self, ctx, global_start):
        """Generate this (slice of the) dictionary in device memory and sweep it."""
        if self.dtype != np.float32:
            # the fused path produces float32 patterns; other dtypes take the reference's
            # route: materialise, then prepare_dictionary casts (cf. .astype(dtype) at
            # similarity_metrics/_normalized_cross_correlation.py:235)
            ctx.push_dictionary_chunk(self.compute(ctx), global_start)
            return
        self.configure(ctx)
        if self.pcs is not None:
            ctx.push_rotations_chunk_varying_pc(self.rotations, self.pcs, global_start, self.detector.detector_to_sample,
                                                self.rescale, self.out_min, self.out_max)
            return
        ctx.push_rotations_chunk(self.rotations, global_start, self.rescale, self.out_min, self.out_max)

    def hold_in_engine(self, ctx, global_start):
        """Generate this (slice of the) dictionary in device memory and keep it prepared there
        (`kikuchipy_amd.ResidentDictionary`)."""
        if self.dtype != np.float32 or self.pcs is not None:
            ctx.hold_dictionary_chunk(self.compute(ctx), global_start)
            return
        self.configure(ctx)
        ctx.hold_rotations_chunk(self.rotations, global_start, self.rescale, self.out_min, self.out_max)

    def compute(self, ctx=None):
        """The patterns as a NumPy array (projected on the GPU)."""
        if ctx is None:
            root = self._root
            if root._ctx is None:
                root._ctx = _lib.Context(self.device)
            ctx = root._ctx
        self.configure(ctx)
        out = np.empty(self.shape, dtype=self.dtype)
        n, step = len(self), self.chunksize[0]
        flat = out.reshape(n, -1)
        for a in range(0, n, step):
            if self.pcs is not None:
                flat[a:a + step] = ctx.project_patterns_varying_pc(self.rotations[a:a + step], self.pcs[a:a + step],
                                                                   self.detector.shape, self.detector.detector_to_sample,
                                                                   self.rescale, self.out_min, self.out_max, self.dtype)
            else:
                flat[a:a + step] = ctx.project_patterns(self.rotations[a:a + step], self.rescale, self.out_min,
                                                        self.out_max, self.dtype)
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.compute()
        return a if dtype is None else a.astype(dtype)

    def __repr__(self):
        return (f"ProjectedDictionary(shape={self.shape}, dtype={self.dtype}, rescale={self.rescale}, "
                f"chunksize={self.chunksize})")


class Reflectors:
    """A list of reflectors for `KikuchiPatternSimulator`: what the simulator reads of diffsims'
    `ReciprocalLatticeVector`, as plain arrays.

    Parameters
    ----------
    hkl
        (m, 3) Miller indices.
    theta
        m Bragg angles in radians, or None (not calculated: NaN, as in diffsims).
    structure_factor
        m (complex) structure factors, or None (not calculated: NaN).
    reciprocal_basis
        (3, 3) rows a*, b*, c* in Cartesian coordinates; the reflectors' Cartesian vectors are `hkl @ reciprocal_basis`.
        None is the identity: a cubic lattice (the unit vectors do not depend on its parameter).
    phase_name, has_inversion_symmetry
        What the master pattern takes over from the phase (`EBSDMasterPattern`).
    """

    def __init__(self, hkl, theta, structure_factor=None, reciprocal_basis=None, phase_name="", has_inversion_symmetry=True):
        self.hkl = np.atleast_2d(np.asarray(hkl, dtype=np.float64))
        if self.hkl.ndim != 2 or self.hkl.shape[1] != 3:
            raise ValueError(f"hkl of shape {np.shape(hkl)}: (m, 3) expected")
        m = self.hkl.shape[0]
        self.theta = np.full(m, np.nan) if theta is None else np.asarray(theta, dtype=np.float64).reshape(-1)
        if structure_factor is None:
            self.structure_factor = np.full(m, np.nan, dtype=np.complex128)
        else:
            self.structure_factor = np.asarray(structure_factor).reshape(-1)
        if self.theta.size != m or self.structure_factor.size != m:
            raise ValueError(f"{m} reflectors but {self.theta.size} Bragg angles and {self.structure_factor.size} "
                             "structure factors")
        basis = np.eye(3) if reciprocal_basis is None else np.asarray(reciprocal_basis, dtype=np.float64)
        if basis.shape != (3, 3):
            raise ValueError(f"reciprocal_basis of shape {basis.shape}: (3, 3) expected")
        self.reciprocal_basis = basis
        self.phase_name = phase_name
        self.has_inversion_symmetry = has_inversion_symmetry

    @property
    def size(self):
        return self.hkl.shape[0]

    @property
    def data(self):
        """Cartesian coordinates of the reciprocal lattice vectors."""
        return self.hkl @ self.reciprocal_basis

    @property
    def unit_vectors(self):
        """`Vector3d(reflectors).unit.data`: the Cartesian vectors divided by sqrt(sum of squares)."""
        data = self.data
        return data / np.sqrt(np.sum(data**2, axis=-1))[:, np.newaxis]

    @property
    def direct_basis(self):
        """(3, 3) rows a, b, c in Cartesian coordinates: `inv(reciprocal_basis.T)`; a direction's Cartesian vector is
        `uvw @ direct_basis`."""
        return np.linalg.inv(self.reciprocal_basis.T)

    def __getitem__(self, key):
        """The reflectors a boolean mask or an index (array, slice) selects, as a new `Reflectors`."""
        if isinstance(key, (int, np.integer)):
            key = [key]
        return Reflectors(self.hkl[key], self.theta[key], self.structure_factor[key], self.reciprocal_basis.copy(),
                          self.phase_name, self.has_inversion_symmetry)

    def deepcopy(self):
        return copy.deepcopy(self)

    def flatten(self):
        return self

    def __repr__(self):
        return (f"Reflectors ({self.size},), {self.phase_name or 'unnamed phase'}\n"
                f"[{', '.join(str(row) for row in self.hkl[:4].astype(int).tolist())}{', ...' if self.size > 4 else ''}]")


def _unit_vectors_of(reflectors):
    """(m, 3) float64 unit normals of a `Reflectors` or of anything shaped like diffsims' `ReciprocalLatticeVector`
    (`unit` being a vector object with `data`)."""
    u = getattr(reflectors, "unit_vectors", None)
    if u is None:
        u = reflectors.unit
        u = getattr(u, "data", u)
    return np.ascontiguousarray(u, dtype=np.float64).reshape(-1, 3)


def _phase_of(reflectors):
    """(phase name, has_inversion_symmetry) of a `Reflectors`, or from the `phase` of a diffsims object."""
    if hasattr(reflectors, "phase_name"):
        return reflectors.phase_name, getattr(reflectors, "has_inversion_symmetry", True)
    phase = getattr(reflectors, "phase", None)
    point_group = getattr(phase, "point_group", None)
    return getattr(phase, "name", "") or "", None if point_group is None else bool(point_group.contains_inversion)


class KikuchiPatternSimulator:
    """Setup and calculation of kinematical Kikuchi pattern simulations.

    Parameters
    ----------
    reflectors
        Reflectors to use in the simulation, flattened to one navigation dimension: a `Reflectors`, or any object with
        `hkl`, `theta`, `structure_factor` and unit vectors (diffsims' `ReciprocalLatticeVector`).
    """

    def __init__(self, reflectors):
        self._reflectors = reflectors.deepcopy().flatten()

    @property
    def reflectors(self):
        """Return the reflectors to use in the simulation."""
        return self._reflectors

    def __repr__(self):
        return f"{self.__class__.__name__}:\n" + repr(self.reflectors)

    def calculate_master_pattern(self, half_size=500, hemisphere="upper", scaling="linear", *, device=0, context=None):
        """Return a kinematical master pattern in the stereographic projection, summed on the GPU.

        `half_size`: the pattern has 2 * half_size + 1 pixels per side; `hemisphere`: "upper", "lower" or "both";
        `scaling` of the band intensities: "linear" |F|, "square" |F|^2, or None (all bands 1).  Returns an
        `EBSDMasterPattern` of float64 data, (size, size) or (2, size, size) for "both", `projection="stereographic"`;
        `as_lambert()` makes it ready for `get_patterns`.  `device` / `context`: the GPU, or a `Context` to run on."""
        self._raise_if_no_theta()
        self._raise_if_no_structure_factor()
        if not isinstance(hemisphere, str) or hemisphere.lower() not in _lib.HEMISPHERE_CODES:
            raise ValueError(f"Unknown hemisphere {hemisphere!r}, options are 'upper', 'lower', or 'both'")
        hemisphere = hemisphere.lower()
        ref = self.reflectors
        if scaling == "linear":
            intensity = abs(np.asarray(ref.structure_factor))
        elif scaling == "square":
            factor = np.asarray(ref.structure_factor)
            intensity = abs(factor * factor.conjugate())
        elif scaling is None:
            intensity = np.ones(ref.size)
        else:
            raise ValueError(f"Unknown scaling {scaling!r}, options are 'linear', 'square', or None")
        from kikuchipy_amd.signals import EBSDMasterPattern

        ctx = context if context is not None else _lib.Context(device)
        try:
            data = ctx.kinematical_master_pattern(_unit_vectors_of(ref), ref.theta, intensity, half_size, hemisphere)
        finally:
            if context is None:
                ctx.close()
        phase_name, inversion = _phase_of(ref)
        return EBSDMasterPattern(data, projection="stereographic", hemisphere=hemisphere, phase_name=phase_name,
                                 has_inversion_symmetry=inversion, device=device)

    def on_detector(self, detector, rotations, *, device=0, context=None):
        """Project Kikuchi lines and zone axes onto a detector, one set per crystal orientation, on the GPU.

        `detector`: an `EBSDDetector` whose `navigation_shape` is (1,) or equal to the shape of `rotations`.
        `rotations`: unit quaternions of shape (n, 4) or (ny, nx, 4), or an object with such `data` (orix' `Rotation`).
        Returns a `GeometricalKikuchiPatternSimulation`.  Reflectors with z > 0 on the detector at no map point are
        dropped; zone axes are the reduced integer cross products of all pairs of the kept reflectors, `[uvw]` and
        `[-u -v -w]` both, in lexicographic order, kept when in some pattern.  `device` / `context`: the GPU, or a
        `Context` to run on."""
        rot = np.asarray(getattr(rotations, "data", rotations), dtype=np.float64)
        if rot.ndim not in (2, 3) or rot.shape[-1] != 4:
            raise ValueError(f"rotations of shape {rot.shape}: unit quaternions (n, 4) or (ny, nx, 4) expected")
        nav_shape = rot.shape[:-1]
        if detector.navigation_shape != (1,) and detector.navigation_shape != nav_shape:
            raise ValueError("`detector.navigation_shape` is not (1,) or equal to `rotations.shape`")
        ref = self.reflectors
        hkl = np.asarray(ref.hkl, dtype=np.float64).reshape(-1, 3)
        a_star = getattr(ref, "reciprocal_basis", None)
        if a_star is None:  # (diffsims: phase.structure.lattice.recbase.T)
            a_star = ref.phase.structure.lattice.recbase.T
        a_star = np.ascontiguousarray(a_star, dtype=np.float64)
        a_direct = np.linalg.inv(a_star.T)
        hkl_int = np.rint(hkl).astype(np.int64)
        if not np.array_equal(hkl_int, hkl):
            raise ValueError("on_detector needs integer Miller indices hkl (zone axes are formed exactly in integers)")
        q = np.ascontiguousarray(rot.reshape(-1, 4))
        u_s = np.ascontiguousarray(detector.detector_to_sample)  # sample_to_detector transposed
        pcs = _geometrical_pc_table(detector)
        r_gnomonic = float(np.max(detector.r_max))
        ctx = context if context is not None else _lib.Context(device)
        try:
            flags = ctx.geometrical_visibility(hkl, _lib.GEOMETRICAL_LINES, q, u_s, a_star, pcs)
            keep = (flags & _lib.GEOMETRICAL_UPPER) != 0
            visible = ref[keep]
            if not keep.any():
                raise ValueError("No reflector is in a pattern: every hkl has z <= 0 on the detector at every map point")
            uvw = zone_axes_from_reflectors(hkl_int[keep])
            if uvw.shape[0]:
                flags = ctx.geometrical_visibility(uvw, _lib.GEOMETRICAL_ZONE_AXES, q, u_s, a_direct, pcs)
                both = _lib.GEOMETRICAL_UPPER | _lib.GEOMETRICAL_INSIDE
                uvw = uvw[(flags & both) == both]
            out = ctx.geometrical_coordinates(hkl[keep], uvw, q, u_s, a_star, a_direct, pcs, r_gnomonic)
        finally:
            if context is None:
                ctx.close()
        chain = (q, u_s, a_star, a_direct)
        lines = KikuchiPatternLine(hkl[keep], chain, nav_shape, out["line_in_pattern"], out["line_gnomonic"], r_gnomonic)
        zone_axes = KikuchiPatternZoneAxis(uvw, chain, nav_shape, out["zone_in_pattern"], out["zone_gnomonic"], r_gnomonic)
        return GeometricalKikuchiPatternSimulation(detector, rot, visible, lines, zone_axes,
                                                   out["line_pixel"].reshape(nav_shape + (-1, 4)),
                                                   out["zone_pixel"].reshape(nav_shape + (-1, 2)))

    def _raise_if_no_theta(self):
        if np.isnan(self.reflectors.theta[0]):
            raise ValueError(
                "Reflectors have no Bragg angles. Calculate with "
                "`diffsims.crystallography.ReciprocalLatticeVector.calculate_theta()`."
            )

    def _raise_if_no_structure_factor(self):
        if np.isnan(self.reflectors.structure_factor[0]):
            raise ValueError(
                "Reflectors have no structure factors. Calculate with "
                "`diffsims.crystallography.ReciprocalLatticeVector."
                "calculate_structure_factor()`."
            )


def zone_axes_from_reflectors(hkl):
    """Zone axes [uvw] of all ordered pairs of the integer reflectors `hkl` (k, 3): the integer cross products (the
    direct-lattice indices of g1 x g2 are proportional to them), without [000], each divided by the gcd of its indices
    (the sign stays: [uvw] and [-u -v -w] are two entries), unique, in lexicographic order.  (z, 3) float64.  Stands in
    for `Miller.cross`, `.round()` and `.unique()` of orix (simulations/kikuchi_pattern_simulator.py:290-297), whose
    output order is not reproduced."""
    hkl = np.asarray(hkl, dtype=np.int64).reshape(-1, 3)
    uvw = np.cross(hkl[:, np.newaxis, :], hkl[np.newaxis, :, :]).reshape(-1, 3)
    uvw = uvw[np.any(uvw != 0, axis=1)]
    if uvw.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.float64)
    uvw = uvw // np.gcd.reduce(np.abs(uvw), axis=1)[:, np.newaxis]
    return np.unique(uvw, axis=0).astype(np.float64)


def _geometrical_pc_table(detector):
    """(1 or n, 8) per projection centre: the gnomonic x and y ranges widened by one pixel, the offsets
    pcx / pcz * aspect_ratio and pcy / pcz, and the pixel scales (simulations/_kikuchi_pattern_simulation.py:473-525)."""
    x_range = detector.x_range.reshape(-1, 2)
    y_range = detector.y_range.reshape(-1, 2)
    x_scale = np.reshape(detector.x_scale, -1)
    y_scale = np.reshape(detector.y_scale, -1)
    pc = detector.pc_flattened
    table = np.empty((pc.shape[0], _lib.GEOMETRICAL_PC_DOUBLES), dtype=np.float64)
    table[:, 0] = x_range[:, 0] - x_scale
    table[:, 1] = x_range[:, 1] + x_scale
    table[:, 2] = y_range[:, 0] - y_scale
    table[:, 3] = y_range[:, 1] + y_scale
    table[:, 4] = (pc[:, 0] / pc[:, 2]) * detector.aspect_ratio
    table[:, 5] = pc[:, 1] / pc[:, 2]
    table[:, 6] = x_scale
    table[:, 7] = y_scale
    return table


def parse_coordinate_format(fmt):
    """detectors/_convert_detector_coordinates.py:39-52 of the reference: "detector" is the deprecated spelling of "pixel"."""
    if fmt == "detector":
        import warnings

        try:
            from numpy.exceptions import VisibleDeprecationWarning
        except ImportError:  # NumPy before 1.25
            from numpy import VisibleDeprecationWarning
        warnings.warn("Pass 'pixel' instead. Passing 'detector' is deprecated and will throw an error in 0.13.0",
                      VisibleDeprecationWarning, stacklevel=2)
        fmt = "pixel"
    if fmt not in ("pixel", "gnomonic"):
        raise ValueError(f"Unknown coordinate format {fmt!r}. Expected 'pixel' or 'gnomonic'.")
    return fmt


class KikuchiPatternFeature:
    """What the lines and the zone axes share (simulations/_kikuchi_pattern_features.py:22-51).  `in_pattern` and the
    coordinates come from the GPU; the scalar features are formed from the vectors in detector coordinates when asked
    for, with the reference's NumPy expressions."""

    def __init__(self, vector, chain, navigation_shape, in_pattern, max_r_gnomonic):
        self.vector = vector
        self._chain = chain
        self._nav = tuple(navigation_shape)
        self.in_pattern = in_pattern.reshape(self._nav + (-1,))
        self.max_r_gnomonic = max_r_gnomonic
        self.ndim = 1

    _basis = 2  # index into the chain: a_star for lines, a_direct for zone axes

    @property
    def vector_detector(self):
        """(navigation shape, n, 3) the features in detector coordinates: vector (basis U_o U_s)."""
        q, u_s = self._chain[:2]
        u_os = rotation_matrices(q) @ u_s
        return (self.vector @ (self._chain[self._basis] @ u_os)).reshape(self._nav + (-1, 3))

    @property
    def x_gnomonic(self):
        v = self.vector_detector
        with np.errstate(divide="ignore", invalid="ignore"):
            return v[..., 0] / v[..., 2]

    @property
    def y_gnomonic(self):
        v = self.vector_detector
        with np.errstate(divide="ignore", invalid="ignore"):
            return v[..., 1] / v[..., 2]

    def _within(self, coordinates):
        with np.errstate(invalid="ignore"):
            return np.logical_and(coordinates < self.max_r_gnomonic, self.vector_detector[..., 2] > -1e-5)


class KikuchiPatternLine(KikuchiPatternFeature):
    """simulations/_kikuchi_pattern_features.py:54-102"""

    def __init__(self, hkl, chain, navigation_shape, in_pattern, plane_trace, max_r_gnomonic=10.0):
        super().__init__(hkl, chain, navigation_shape, in_pattern, max_r_gnomonic)
        self._plane_trace_coordinates = plane_trace.reshape(self._nav + (-1, 4))

    hkl = property(lambda self: self.vector)

    def _cot_polar(self):
        v = self.vector_detector
        with np.errstate(divide="ignore", invalid="ignore"):
            return v[..., 2] / np.sqrt(v[..., 0] ** 2 + v[..., 1] ** 2)

    @property
    def within_r_gnomonic(self):
        return self._within(np.abs(self._cot_polar()))

    @property
    def hesse_distance(self):
        """tan(pi/2 - polar) = z / sqrt(x^2 + y^2), NaN where not within (as the reference leaves it)."""
        return np.where(self.within_r_gnomonic, self._cot_polar(), np.nan)

    @property
    def hesse_alpha(self):
        return np.arccos(self.hesse_distance / self.max_r_gnomonic)

    @property
    def plane_trace_coordinates(self):
        """x0, y0, x1, y1"""
        return self._plane_trace_coordinates


class KikuchiPatternZoneAxis(KikuchiPatternFeature):
    """simulations/_kikuchi_pattern_features.py:105-129"""

    _basis = 3

    def __init__(self, uvw, chain, navigation_shape, in_pattern, xy, max_r_gnomonic=10.0):
        super().__init__(uvw, chain, navigation_shape, in_pattern, max_r_gnomonic)
        self._xy_within_r_gnomonic = xy.reshape(self._nav + (-1, 2))

    uvw = property(lambda self: self.vector)

    @property
    def r_gnomonic(self):
        return np.sqrt(self.x_gnomonic**2 + self.y_gnomonic**2)

    @property
    def within_r_gnomonic(self):
        return self._within(self.r_gnomonic)


def rotation_matrices(q):
    """(n, 3, 3) matrices of unit quaternions (n, 4): orix' `Rotation.to_matrix`, the matrix of `rotate_vector`
    (_utils/numba.py:62-81 of the reference; csrc/projection.h, csrc/geometrical_plan.h)."""
    a, b, c, d = (q[:, i] for i in range(4))
    aa, bb, cc, dd = a * a, b * b, c * c, d * d
    return np.stack([aa + bb - cc - dd, 2.0 * (b * c - a * d), 2.0 * (a * c + b * d),
                     2.0 * (a * d + b * c), aa - bb + cc - dd, 2.0 * (c * d - a * b),
                     2.0 * (b * d - a * c), 2.0 * (a * b + c * d), aa - bb - cc + dd], axis=-1).reshape(-1, 3, 3)


class GeometricalKikuchiPatternSimulation:
    """Coordinates of Kikuchi lines and zone axes on an EBSD detector, one set per crystal orientation
    (simulations/_kikuchi_pattern_simulation.py:44-534 of the reference).  Returned from
    `KikuchiPatternSimulator.on_detector`, not meant to be created directly.  `lines_coordinates` and
    `zone_axes_coordinates` give what a plot is fed with; `as_collections`, `as_markers` and `plot` need Matplotlib /
    HyperSpy and are not part of this package."""

    def __init__(self, detector, rotations, reflectors, lines, zone_axes, lines_detector_coordinates,
                 zone_axes_detector_coordinates):
        self._detector = detector.deepcopy()
        self._rotations = np.array(rotations, dtype=np.float64)
        self._reflectors = reflectors.deepcopy()
        self._lines = lines
        self._zone_axes = zone_axes
        self._lines_detector_coordinates = lines_detector_coordinates
        self._zone_axes_detector_coordinates = zone_axes_detector_coordinates
        self.ndim = self._rotations.ndim - 1

    @property
    def detector(self):
        """Return the EBSD detector onto which simulations were generated."""
        return self._detector

    @property
    def rotations(self):
        """Return the crystal orientations (unit quaternions) for which simulations were generated."""
        return self._rotations

    @property
    def reflectors(self):
        """Return the reflectors used in the simulations: those in some pattern."""
        return self._reflectors

    @property
    def navigation_shape(self):
        """Return the navigation shape of the simulations, the shape of `rotations` without the quaternion axis."""
        return self._rotations.shape[:-1]

    @property
    def lines(self):
        """The Kikuchi lines' features: `in_pattern`, `within_r_gnomonic`, `hesse_distance`, `hesse_alpha`,
        `plane_trace_coordinates`, `x_gnomonic`, `y_gnomonic`."""
        return self._lines

    @property
    def zone_axes_features(self):
        """The zone axes' features: `in_pattern`, `within_r_gnomonic`, `r_gnomonic`, `x_gnomonic`, `y_gnomonic`."""
        return self._zone_axes

    @property
    def zone_axes(self):
        """(z, 3) the zone axes [uvw] in some pattern, in lexicographic order."""
        return self._zone_axes.vector

    def __repr__(self):
        return f"{self.__class__.__name__} {self.navigation_shape}:\n" + repr(self.reflectors)

    def _coordinates(self, index, coordinates, exclude_nan, pixel, gnomonic):
        coordinates = parse_coordinate_format(coordinates)
        if index is None:
            index = (0, 0)[: self.ndim]
        coords = (pixel if coordinates == "pixel" else gnomonic)[index]
        if exclude_nan:
            coords = coords[~np.isnan(coords).any(axis=-1)]
        return coords.copy()

    def lines_coordinates(self, index=None, coordinates="pixel", exclude_nan=True):
        """Return Kikuchi line coordinates (x0, y0, x1, y1) for a single simulation: `index` of the simulation (the first
        if not given), `coordinates` "pixel" (default) or "gnomonic", `exclude_nan` whether to leave out lines not present
        in the pattern (if False, every index returns an array of the same shape)."""
        return self._coordinates(index, coordinates, exclude_nan, self._lines_detector_coordinates,
                                 self._lines.plane_trace_coordinates)

    def zone_axes_coordinates(self, index=None, coordinates="pixel", exclude_nan=True):
        """Return zone axes coordinates (x, y) for a single simulation; parameters as in `lines_coordinates`."""
        return self._coordinates(index, coordinates, exclude_nan, self._zone_axes_detector_coordinates,
                                 self._zone_axes._xy_within_r_gnomonic)

    def _no_plotting(self, name):
        raise NotImplementedError(f"`{name}` needs Matplotlib / HyperSpy, which this package does not use: feed a plot with "
                                  "`lines_coordinates()` and `zone_axes_coordinates()`")

    def as_collections(self, index=None, coordinates="pixel", lines=True, zone_axes=False, zone_axes_labels=False,
                       lines_kwargs=None, zone_axes_kwargs=None, zone_axes_labels_kwargs=None):
        self._no_plotting("as_collections")

    def as_markers(self, lines=True, zone_axes=False, zone_axes_labels=False, pc=False, lines_kwargs=None,
                   zone_axes_kwargs=None, zone_axes_labels_kwargs=None, pc_kwargs=None):
        self._no_plotting("as_markers")

    def plot(self, index=None, coordinates="pixel", pattern=None, lines=True, zone_axes=True, zone_axes_labels=True, pc=True,
             pattern_kwargs=None, lines_kwargs=None, zone_axes_kwargs=None, zone_axes_labels_kwargs=None, pc_kwargs=None,
             return_figure=False):
        self._no_plotting("plot")
