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
