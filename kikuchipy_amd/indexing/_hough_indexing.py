"""Hough indexing on the GPU engine: `EBSDDetector.get_indexer`, `EBSD.hough_indexing`,
`EBSD.hough_indexing_optimize_pc` and `xmap_from_hough_indexing_data` (DESIGN.md sections 26 and 28; csrc/hough.hip,
csrc/hough_plan.h, csrc/hough_vote.h, csrc/hough_search.h).

The reference hands these calls to PyEBSDIndex (indexing/_hough_indexing.py, signals/ebsd.py:1600-1825 of the reference),
which is not available to this project: the interface - the names, the attributes the reference reads from an indexer,
the field names of the returned arrays, the checks and their error texts - is the reference's, the algorithm behind it
is this package's own, and its numbers are NOT PyEBSDIndex's.  Three kernels: the Radon transform of the patterns, band
detection in the sinograms, and indexing of the bands by triplet voting and an orthogonal fit.

A phase is a `HoughPhase`: the reflectors of a `simulations.Reflectors` taken as lines (g and -g are one), completed
under the proper operations of a point group (`sampling.rotation_group_name`) when one is named, grouped into families
of equal |g|, with the table of their interplanar angles.  Any lattice works through `Reflectors.reciprocal_basis`."""

import time

import numpy as np

from kikuchipy_amd import _lib, sampling
from kikuchipy_amd.indexing._dictionary_indexing import MapData

__all__ = ["HoughIndexer", "HoughPhase", "HoughIndexingResult", "xmap_from_hough_indexing_data"]

DEFAULT_CUBIC_FAMILIES = ((1, 1, 1), (2, 0, 0), (2, 2, 0), (3, 1, 1))  # what the reference's default indexes fcc with
INDEX_DTYPE = np.dtype([("quat", "<f8", (4,)), ("iq", "<f4"), ("pq", "<f4"), ("cm", "<f4"), ("phase", "<i4"), ("fit", "<f4"),
                        ("nmatch", "<i4"), ("matchattempts", "<i4", (2,)), ("totvotes", "<i4")])
MAX_TOLERANCE = np.deg2rad(5.0)


def _rotation_matrices(q):
    a, b, c, d = (q[:, i] for i in range(4))
    return np.stack([np.stack([a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)], -1),
                     np.stack([2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)], -1),
                     np.stack([2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d], -1)], -2)


class HoughPhase:
    """One phase as the indexing kernel takes it: `normals` (n, 3) unit vectors of the reflector lines in crystal
    Cartesian coordinates, `family` (n,) int32, `angles` (n, n) folded interplanar angles in radians, `lengths` (n,)."""

    def __init__(self, reflectors, point_group=None, name=None):
        from kikuchipy_amd.simulations import Reflectors

        if not hasattr(reflectors, "reciprocal_basis"):
            reflectors = Reflectors(np.asarray(reflectors, dtype=np.float64), None)
        self.reflectors = reflectors
        self.point_group = None if point_group is None else getattr(point_group, "name", point_group)
        self.phasename = name if name is not None else (reflectors.phase_name or "")
        g = np.asarray(reflectors.data, dtype=np.float64).reshape(-1, 3)
        if self.point_group is not None:
            ops = sampling.rotation_group_operations(sampling.rotation_group_name(self.point_group))
            g = np.einsum("sij,pj->psi", _rotation_matrices(np.asarray(ops, dtype=np.float64)), g).reshape(-1, 3)
        length = np.sqrt(np.sum(g * g, axis=1))
        if g.shape[0] == 0 or not np.all(np.isfinite(length)) or np.any(length == 0):
            raise ValueError("reflectors must be finite vectors other than [000]")
        u = g / length[:, None]
        u[np.abs(u) < 1e-12] = 0.0
        lead = np.zeros(len(u))
        for k in (2, 1, 0):
            lead = np.where(u[:, k] != 0, u[:, k], lead)
        u = np.where((lead < 0)[:, None], -u, u)
        _, first = np.unique(np.round(u, 9), axis=0, return_index=True)
        keep = np.sort(first)
        self.normals = np.ascontiguousarray(u[keep])
        self.lengths = length[keep]
        scale = self.lengths.max()
        _, fam_first, fam = np.unique(np.round(self.lengths / scale, 9), return_index=True, return_inverse=True)
        order = np.argsort(np.argsort(fam_first))  # families numbered by first appearance
        self.family = order[fam].astype(np.int32)
        if self.normals.shape[0] > _lib.HOUGH_MAX_REFLECTORS or int(self.family.max()) + 1 > _lib.HOUGH_MAX_FAMILIES:
            raise ValueError(f"{self.normals.shape[0]} reflector lines in {int(self.family.max()) + 1} families: Hough indexing "
                             f"takes at most {_lib.HOUGH_MAX_REFLECTORS} in {_lib.HOUGH_MAX_FAMILIES}; pass the strongest families")
        self.angles = np.arccos(np.clip(np.abs(self.normals @ self.normals.T), 0.0, 1.0))

    @property
    def latticeparameter(self):
        """(a, b, c, alpha, beta, gamma) of the direct lattice, angles in degrees."""
        d = self.reflectors.direct_basis
        n = np.sqrt(np.sum(d * d, axis=1))
        cos = [d[1] @ d[2] / (n[1] * n[2]), d[0] @ d[2] / (n[0] * n[2]), d[0] @ d[1] / (n[0] * n[1])]
        return tuple(float(v) for v in n) + tuple(float(np.degrees(np.arccos(np.clip(c, -1, 1)))) for c in cos)

    def __repr__(self):
        return f"HoughPhase {self.phasename or 'unnamed'}: {self.normals.shape[0]} lines in {int(self.family.max()) + 1} families"


def _phases(phase_list, reflectors=None):
    """A list of `HoughPhase` from what `get_indexer` and `hough_indexing` take as a phase list: a `HoughPhase`, a
    `Reflectors`, a (`Reflectors` or hkl array, point group) pair, or a point-group name (a cubic lattice indexed with
    `reflectors` or {111}, {200}, {220}, {311}) - one of these, or a list of them."""
    if isinstance(phase_list, (HoughPhase, str)) or hasattr(phase_list, "reciprocal_basis") or (
            isinstance(phase_list, tuple) and len(phase_list) == 2 and isinstance(phase_list[1], str)):
        phase_list = [phase_list]
    phase_list = list(phase_list)
    if reflectors is None:
        reflectors = [None] * len(phase_list)
    elif isinstance(reflectors, np.ndarray) or hasattr(reflectors, "reciprocal_basis") or len(reflectors) != len(phase_list):
        reflectors = [reflectors]
    if len(reflectors) != len(phase_list):
        raise ValueError("One set of reflectors or None must be passed per phase in the phase list.")
    out = []
    for phase, ref in zip(phase_list, reflectors):
        if isinstance(phase, HoughPhase):
            out.append(phase)
        elif isinstance(phase, str):
            out.append(HoughPhase(DEFAULT_CUBIC_FAMILIES if ref is None else ref, phase))
        elif isinstance(phase, tuple):
            out.append(HoughPhase(phase[0] if ref is None else ref, phase[1]))
        else:
            out.append(HoughPhase(phase if ref is None else ref))
    return out


class _BandDetectPlan:
    def __init__(self, shape, nBands, nTheta, nRho, tSigma, rSigma, rhoMaskFrac):
        self.patDim = tuple(int(v) for v in shape)
        ny, nx = self.patDim
        self.nBands, self.nTheta = int(nBands), int(nTheta)
        self.nRho = _lib.hough_default_n_rho(ny, nx) if nRho is None else int(nRho)
        self.tSigma = self.nTheta / 180.0 if tSigma is None else float(tSigma)
        self.rSigma = min(ny, nx) / 60.0 * (self.nRho / _lib.hough_default_n_rho(ny, nx)) if rSigma is None else float(rSigma)
        self.rhoMaskFrac = float(rhoMaskFrac)
        if not 1 <= self.nBands <= _lib.HOUGH_MAX_BANDS:
            raise ValueError(f"nBands {nBands}: between 1 and {_lib.HOUGH_MAX_BANDS}")

    def tables(self):
        """What the band kernels take from the host, as float32: (cos, sin)(a pi / nTheta) of shape (2, nTheta); the taps
        along theta, a normalised Gaussian of `tSigma` cells; the taps along rho, a normalised Gaussian of `rSigma`
        cells minus one of twice the width - a band-pass that answers to a bright band between its dark edges and not
        to the slow background that is left in an experimental pattern (radius ceil(3 sigma) of the wider Gaussian, 16
        cells at the most; one tap for sigma <= 0); and the number of cells at either end of the rho axis that hold no
        band, max(1, int(rhoMaskFrac nRho))."""
        theta = np.arange(self.nTheta) * np.pi / self.nTheta
        cos_sin = np.stack([np.cos(theta), np.sin(theta)]).astype(np.float32)

        def gauss(sigma, radius):
            d = np.arange(-radius, radius + 1, dtype=np.float64)
            w = np.exp(-0.5 * (d / sigma) ** 2)
            return w / w.sum()

        one = np.ones(1, dtype=np.float32)
        wt = gauss(self.tSigma, min(int(np.ceil(3.0 * self.tSigma)), 16)).astype(np.float32) if self.tSigma > 0 else one
        radius = min(int(np.ceil(6.0 * self.rSigma)), 16) if self.rSigma > 0 else 0
        wr = (gauss(self.rSigma, radius) - gauss(2.0 * self.rSigma, radius)).astype(np.float32) if radius else one
        return cos_sin, wt, wr, max(1, int(self.rhoMaskFrac * self.nRho))

    @property
    def rho_cell(self):
        """Pixels per rho cell."""
        return 2.0 * np.floor((min(self.patDim) - 1) / 2.0) / (self.nRho - 1)


class HoughIndexer:
    """What `EBSDDetector.get_indexer` returns, with the attributes the reference reads from PyEBSDIndex's `EBSDIndexer`:
    `PC`, `sampleTilt`, `camElev`, `vendor`, `phaselist`, `bandDetectPlan.patDim` and `.nBands`."""

    def __init__(self, phaselist, shape, PC=(0.5, 0.5, 0.5), sampleTilt=70.0, camElev=0.0, vendor="KIKUCHIPY", *, nBands=9,
                 nTheta=180, nRho=None, tSigma=None, rSigma=None, rhoMaskFrac=0.1):
        self.phaselist = list(phaselist)
        self.PC = np.asarray(PC, dtype=np.float64)
        self.sampleTilt, self.camElev, self.vendor = float(sampleTilt), float(camElev), vendor
        self.bandDetectPlan = _BandDetectPlan(shape, nBands, nTheta, nRho, tSigma, rSigma, rhoMaskFrac)

    def tolerance(self, pcs):
        """The angular tolerance of the vote in radians: two sinogram cells - the larger of a rho cell seen from the
        source point, atan(cell / (PCz Ny)), and a theta cell - and 5 degrees at the most."""
        plan = self.bandDetectPlan
        pcz = float(np.mean(np.asarray(pcs, dtype=np.float64).reshape(-1, 3)[:, 2]))
        cell = max(np.arctan(plan.rho_cell / (pcz * plan.patDim[0])), np.pi / plan.nTheta)
        return float(min(2.0 * cell, MAX_TOLERANCE))

    @property
    def sample_to_detector(self):
        from kikuchipy_amd.detectors import sample_to_detector_matrix

        return sample_to_detector_matrix(self.sampleTilt, self.camElev, 0.0, 0.0)

    def detect_bands(self, patterns, context, return_sinograms=False):
        """`band_data` (n, nBands) of `_lib.HOUGH_BAND_DTYPE` of a stack of patterns (host array or resident)."""
        from kikuchipy_amd.pattern import _pattern

        p = self.bandDetectPlan
        cos_sin, wt, wr, rim = p.tables()
        out = _pattern._process(patterns, lambda c: None, context, 0, None, collect=lambda c: c.hough_bands(
            p.nRho, cos_sin, wt, wr, rim, p.nBands, return_sinograms))
        return out

    def index_bands(self, band_data, pcs, context):
        """`index_data` (n_phases + 1, n) of `INDEX_DTYPE` from `band_data`: row p is phase p, the last row the better
        phase per pattern - more matched bands, then the smaller fit, then the first."""
        band_data = np.ascontiguousarray(band_data, dtype=_lib.HOUGH_BAND_DTYPE)
        m = band_data.shape[0]
        pcs = np.asarray(pcs, dtype=np.float64).reshape(-1, 3)
        tol = self.tolerance(pcs)
        out = np.zeros((len(self.phaselist) + 1, m), dtype=INDEX_DTYPE)
        valid = band_data["valid"] != 0
        n_valid = np.maximum(valid.sum(axis=1), 1)
        pq = (np.where(valid, band_data["value"], 0).sum(axis=1) / n_valid).astype(np.float32)
        iq = np.where(valid, band_data["value"], 0).max(axis=1).astype(np.float32)
        for p, phase in enumerate(self.phaselist):
            quat, fit, cm, nmatch = context.hough_index(band_data, pcs, self.bandDetectPlan.patDim, self.sample_to_detector,
                                                        phase.normals, phase.family, phase.angles, tol)
            row = out[p]
            row["quat"], row["fit"], row["cm"], row["nmatch"] = quat, fit, cm, nmatch
            row["phase"] = np.where(nmatch > 0, p, -1)
            row["pq"], row["iq"] = pq, iq
        best = np.lexsort((np.arange(len(self.phaselist))[:, None] + np.zeros(m, dtype=int), out[:-1]["fit"],
                           -out[:-1]["nmatch"]), axis=0)[0]
        out[-1] = out[best, np.arange(m)]
        return out


def indexer_from_detector(detector, phase_list, reflectors=None, **kwargs):
    """`EBSDDetector.get_indexer` (detectors/_ebsd_detector.py:1598 of the reference)."""
    allowed = ("nBands", "nTheta", "nRho", "tSigma", "rSigma", "rhoMaskFrac")
    for key in kwargs:
        if key not in allowed:
            raise TypeError(f"get_indexer() got an unexpected keyword argument {key!r}: the band detection takes {allowed}")
    pc = detector.pc_flattened
    return HoughIndexer(_phases(phase_list, reflectors), detector.shape, pc[0] if pc.shape[0] == 1 else pc, detector.sample_tilt,
                        detector.tilt, "KIKUCHIPY", **kwargs)


# ---- the reference's checks, with its texts (indexing/_hough_indexing.py:339-490) -----------------------------------------
def _indexer_is_compatible_with_kikuchipy(indexer, sig_shape, nav_size=None, check_pc=True, raise_if_not=False):
    compatible, error_msg = True, None
    if indexer.vendor.lower() != "kikuchipy":
        compatible = False
        error_msg = f"'indexer.vendor' must be 'kikuchipy', but was {indexer.vendor}"
    sig_shape_indexer = tuple(map(int, indexer.bandDetectPlan.patDim))
    if compatible and tuple(sig_shape) != sig_shape_indexer:
        compatible = False
        error_msg = f"Indexer signal shape {sig_shape_indexer} must be equal to the signal shape {tuple(sig_shape)}."
    if check_pc:
        pc_shape = np.shape(indexer.PC)
        allowed_shapes, allowed_shapes_str = [(3,)], "(3,)"
        if nav_size is not None:
            allowed_shapes.append((nav_size, 3))
            allowed_shapes_str += f" or ({nav_size}, 3)"
        if compatible and (len(pc_shape) > 2 or pc_shape not in allowed_shapes):
            compatible = False
            error_msg = f"`indexer.PC` must be an array of shape {allowed_shapes_str}, but was {pc_shape} instead."
    if raise_if_not and not compatible:
        raise ValueError(error_msg)
    return compatible


def _phase_lists_are_compatible(phase_list, indexer, raise_if_not=False):
    """Equal numbers of phases in the same order with equal lattice parameters (the reference also compares space group
    numbers, which a `HoughPhase` does not have: the point groups are compared)."""
    phases, theirs = _phases(phase_list), indexer.phaselist
    compatible = True
    msg = f"`indexer.phaselist` {theirs} and the list determined from `phase_list` must be the same"
    if len(phases) != len(theirs):
        compatible = False
        msg = f"`phase_list` ({len(phases)}) and `indexer.phaselist` ({len(theirs)}) have unequal number of phases"
    else:
        for i, (phase, other) in enumerate(zip(phases, theirs)):
            lat, lat_pei = phase.latticeparameter, other.latticeparameter
            if not np.allclose(lat, lat_pei, atol=1e-12):
                compatible = False
                msg = (f"Phase '{phase.phasename}' in `phase_list` and phase number {i} in `indexer.phaselist` have unequal "
                       f"lattice parameters {lat} and {lat_pei}")
                break
            if sampling.rotation_group_name(phase.point_group or "1") != sampling.rotation_group_name(other.point_group or "1"):
                compatible = False
                msg = (f"Phase '{phase.phasename}' in `phase_list` and phase number {i} in `indexer.phaselist` have unequal "
                       f"point groups {phase.point_group} and {other.point_group}")
                break
    if raise_if_not and not compatible:
        raise ValueError(msg)
    return compatible


# ---- results ----------------------------------------------------------------------------------------------------------------
class HoughIndexingResult(MapData):
    """What the reference puts into the `CrystalMap` of `xmap_from_hough_indexing_data`: per map point `rotations`
    (quaternions; the identity where not indexed), `phase_id` (-1: not indexed) and the properties `fit`, `cm`, `pq` and
    `nmatch`; `is_in_data` is all true, `shape` the navigation shape."""

    def __init__(self, rotations, phase_id, prop, nav_shape, step_sizes=None, scan_unit="px", phase_list=None):
        self.rotations, self.phase_id, self.prop = rotations, phase_id, prop
        for key, value in prop.items():
            setattr(self, key, value)
        self.shape = tuple(nav_shape)
        self.is_in_data = np.ones(rotations.shape[0], dtype=bool)
        self.step_sizes, self.scan_unit, self.phase_list = step_sizes, scan_unit, phase_list

    @property
    def size(self):
        return int(self.rotations.shape[0])

    def __repr__(self):
        return f"HoughIndexingResult {self.shape}: {int((self.phase_id >= 0).sum())} of {self.size} points indexed"


def xmap_from_hough_indexing_data(data, phase_list, data_index=-1, navigation_shape=None, step_sizes=None, scan_unit="px"):
    """indexing/_hough_indexing.py:43-118 of the reference: the result holder of row `data_index` of an `index_data`
    array (-1: the better phase per point)."""
    if navigation_shape is None:
        navigation_shape = (data.shape[1],)
    elif len(navigation_shape) > 2 or not all(isinstance(n_i, (int, np.integer)) for n_i in navigation_shape):
        raise ValueError("`nav_shape` cannot be a tuple of more than two integers")
    phase_ids = list(range(len(_phases(phase_list))))
    if data_index != -1 and data_index not in phase_ids:
        raise ValueError(f"`phase_list` IDs {phase_ids} must contain {data_index}")
    row = data[data_index]
    phase_id = np.array(row["phase"])
    rot = np.array(row["quat"], dtype=np.float64)
    rot[phase_id == -1] = [1, 0, 0, 0]
    prop = {name: np.array(row[name]) for name in ("fit", "cm", "pq", "nmatch")}
    return HoughIndexingResult(rot, phase_id, prop, navigation_shape, step_sizes, scan_unit, phase_list)


# ---- the two signal methods -----------------------------------------------------------------------------------------------
def _stack(signal):
    """(patterns as a stack - resident where the signal is -, signal shape, navigation shape, navigation size)."""
    sig, nav = tuple(signal._signal_shape_rc), tuple(signal._navigation_shape_rc)
    if signal.is_resident:
        return signal._resident.flat(), sig, nav, max(signal.navigation_size, 1)
    data = signal.data
    if hasattr(data, "compute"):
        raise NotImplementedError("Hough indexing of lazy signals is not implemented: compute the data first")
    return np.asarray(data).reshape((-1,) + sig), sig, nav, max(signal.navigation_size, 1)


def hough_indexing(signal, phase_list, indexer, chunksize=528, verbose=1, return_index_data=False, return_band_data=False):
    """`EBSD.hough_indexing` (signals/ebsd.py:1600-1719 of the reference).  `chunksize` is accepted and has nothing to
    size: the kernels walk the patterns in passes sized from the free device memory."""
    patterns, sig, nav, nav_size = _stack(signal)
    _indexer_is_compatible_with_kikuchipy(indexer, sig, nav_size, raise_if_not=True)
    _phase_lists_are_compatible(phase_list, indexer, raise_if_not=True)
    tic = time.time()
    band_data = indexer.detect_bands(patterns, signal.context)
    index_data = indexer.index_bands(band_data, indexer.PC, signal.context)
    if verbose:
        pc = np.asarray(indexer.PC, dtype=np.float64).reshape(-1, 3).mean(axis=0).round(4)
        print(f"Hough indexing on the GPU:\n  Projection center (Bruker{', mean' if np.size(indexer.PC) > 3 else ''}): "
              f"{tuple(map(float, pc))}\n  Indexing {nav_size} pattern(s)\n"
              f"  Indexing speed: {nav_size / max(time.time() - tic, 1e-9):.5f} patterns/s")
    xmap = xmap_from_hough_indexing_data(index_data, phase_list, navigation_shape=nav or (1,), step_sizes=signal.step_sizes,
                                         scan_unit=signal.scan_unit)
    out = (xmap,) + ((index_data,) if return_index_data else ()) + ((band_data,) if return_band_data else ())
    return out[0] if len(out) == 1 else out


def _device_search_options(kwargs):
    """The keywords of `hough_indexing_optimize_pc(batch=True)` as the search kernel takes them - dict(xatol, fatol,
    maxiter, maxfev) -, or None where SciPy has to run the search on the host: anything but `tol` and `options` within
    xatol, fatol, maxiter, maxfev and a false disp (`bounds`, `callback`, `adaptive`, `initial_simplex`, `return_all`, a true
    `disp`, a budget of more than `_lib.HOUGH_SEARCH_MAX_EVALS` evaluations per search, ...), and every call under
    KPDI_HOUGH_PC_SEARCH=host.  The parsing is that of `_nelder_mead_options` of the refinement."""
    import os

    if os.environ.get("KPDI_HOUGH_PC_SEARCH", "").lower() == "host":
        return None
    kwargs = dict(kwargs)
    options = dict(kwargs.pop("options", None) or {})
    tol = kwargs.pop("tol", None)
    if kwargs or set(options) - {"xatol", "fatol", "maxiter", "maxfev", "disp"}:
        return None
    # (`tol`: scipy.optimize.minimize lets it set xatol and fatol only where the options name none, and the host path
    # below names both, 1e-3 by default, before SciPy looks: it changes nothing there, so nothing here)
    del tol
    if options.get("disp"):
        return None  # SciPy prints its termination message and warns when the budget runs out: the kernel is silent
    budget = [options.get("maxiter"), options.get("maxfev")]
    if any(v is not None and (not isinstance(v, (int, np.integer)) or v < 1) for v in budget):
        return None  # (SciPy takes infinities and floats too: its business)
    # the kernel refuses a budget that lets one search run on without a sane end (csrc/hough_plan.h); on the host every
    # step is a launch of its own
    most = budget[1] if budget[1] is not None else (600 if budget[0] is None else 4 + 5 * int(budget[0]))
    if most > _lib.HOUGH_SEARCH_MAX_EVALS:
        return None
    return dict(xatol=float(options.get("xatol", 1e-3)), fatol=float(options.get("fatol", 1e-3)), maxiter=budget[0], maxfev=budget[1])


def _host_search(ctx, bands, pc0, args, **kwargs):
    """SciPy's Nelder-Mead on the host over the mean objective of `bands` (k, n_bands), each step one launch of the
    indexing kernel; `args`: what `Context.hough_index` takes after the PC, the tolerance last.  Returns SciPy's
    `OptimizeResult`.  xatol = fatol = 1e-3 unless the options name them."""
    from scipy.optimize import minimize

    kwargs = dict(kwargs)
    options = dict(kwargs.pop("options", None) or {})
    options.setdefault("xatol", 1e-3)
    options.setdefault("fatol", 1e-3)
    tol_deg = float(np.degrees(args[-1]))
    n_valid = (bands["valid"] != 0).sum(axis=1)

    def objective(pc):
        # the mean fit, with every band that found no reflector charged the tolerance: a PC under which bands stop
        # matching must not look better for it (where all bands match this IS the mean fit)
        if not pc[2] > 0:
            return 180.0
        _, fit, _, nmatch = ctx.hough_index(bands, pc, *args)
        charged = np.where(nmatch > 0, fit * nmatch, 0.0) + tol_deg * (n_valid - nmatch)
        return float(np.mean(np.where(n_valid > 0, charged / np.maximum(n_valid, 1), tol_deg)))

    return minimize(objective, pc0, method="Nelder-Mead", options=options, **kwargs)


def hough_indexing_optimize_pc(signal, pc0, indexer, batch=False, method="Nelder-Mead", **kwargs):
    """`EBSD.hough_indexing_optimize_pc` (signals/ebsd.py:1721-1825 of the reference): the bands are detected once, a
    Nelder-Mead search over the PC runs only the indexing, on the first phase, and minimises the mean `fit` - every
    unmatched band counted at the tolerance of the vote - of all patterns, or with `batch` of each pattern on its own.

    With `batch` and plain keywords (`_device_search_options`) every pattern's search runs on the device, one lane per
    pattern, SciPy's Nelder-Mead restated bit for bit (`Context.hough_optimize_pc`).  Otherwise
    the search is `scipy.optimize.minimize` on the host, which takes `**kwargs`, and each step one launch of the
    indexing kernel: `batch=False` (one search over the mean of all patterns), keywords the kernel does not know, and
    every call under KPDI_HOUGH_PC_SEARCH=host.  Both paths return the same bits."""
    from kikuchipy_amd.detectors import EBSDDetector

    pc0 = np.asarray(pc0)
    if pc0.size != 3:
        raise ValueError("`pc0` must be of size 3")
    pc0 = np.asarray(pc0, dtype=np.float64).reshape(3)
    supported_methods = ["nelder-mead", "pso"]
    method = method.lower()
    if method not in supported_methods:
        raise ValueError(f"`method` '{method}' must be one of the supported methods {supported_methods}")
    patterns, sig, nav, nav_size = _stack(signal)
    _indexer_is_compatible_with_kikuchipy(indexer, sig, nav_size, check_pc=False, raise_if_not=True)
    if method == "pso":
        raise NotImplementedError("method 'PSO' (particle swarm) is not implemented: use 'Nelder-Mead'")
    ctx = signal.context
    band_data = indexer.detect_bands(patterns, ctx)
    phase = indexer.phaselist[0]
    tol = indexer.tolerance(pc0)
    args = (indexer.bandDetectPlan.patDim, indexer.sample_to_detector, phase.normals, phase.family, phase.angles, tol)
    device = _device_search_options(kwargs) if batch else None
    if device is not None:
        pc = ctx.hough_optimize_pc(band_data, pc0, *args, **device)[0].reshape(nav + (3,))
        return EBSDDetector(shape=sig, pc=pc, sample_tilt=indexer.sampleTilt, tilt=indexer.camElev)
    if batch:
        pc = np.stack([_host_search(ctx, band_data[i:i + 1], pc0, args, **kwargs).x for i in range(band_data.shape[0])])
        pc = pc.reshape(nav + (3,))
    else:
        pc = _host_search(ctx, band_data, pc0, args, **kwargs).x
    return EBSDDetector(shape=sig, pc=pc, sample_tilt=indexer.sampleTilt, tilt=indexer.camElev)
