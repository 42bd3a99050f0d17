"""Minimal `EBSD` / `EBSDMasterPattern` holders with the methods of the accelerated path.

NOT a re-implementation of kikuchipy's HyperSpy signal (out of scope): just
enough object surface - `data`, `static_background`, `xmap` (dictionary
rotations), the navigation/signal shapes - for the three methods to read like
the reference's:

* `EBSD.remove_static_background`   signals/ebsd.py:442-573
* `EBSD.remove_dynamic_background`  signals/ebsd.py:575-696
* `EBSD.dictionary_indexing`        signals/ebsd.py:1827-1984
* `EBSDMasterPattern.get_patterns`  signals/ebsd_master_pattern.py:95-330
* `EBSD.refine_orientation` / `refine_projection_center` /
  `refine_orientation_projection_center`   signals/ebsd.py:1986-2700

A signal is host-backed by default: like the reference's methods, each call then hands back host data (`self.data`
is replaced by the processed array), which costs an upload and a download per call.  `EBSD.to_device()` makes the
signal resident instead: the patterns live in the HBM of the signal's engine context, every method above and every
pre-processing method works on them where they are (`inplace=True` moves no pattern at all, `inplace=False` copies
device to device into a new resident signal), selections (`inav`, `isig`, `crop`, `extract_grid`) run as a gather on
the GPU, `dictionary_indexing` matches them without an upload, and `data` downloads lazily.  Who owns the buffer and
what invalidates the host copy: DESIGN.md section 20.  `EBSD.sum` / `mean` / `max` / `min` / `std` / `var` reduce over
any set of axes where the patterns are; only the small result comes back.
"""

import copy
import numbers
import warnings

import numpy as np

from kikuchipy_amd import _lib, _selection
from kikuchipy_amd.indexing._dictionary_indexing import dictionary_indexing as _dictionary_indexing
from kikuchipy_amd.pattern import _decomposition, _neighbours, _pattern
from kikuchipy_amd.simulations import DTYPE_RANGE, ProjectedDictionary


# a call that names no device spreads a refinement over every visible GPU from this many points on (one block of the
# points per GPU; below, the set-up of a group costs more than it saves)
REFINE_GROUP_MIN_POINTS = 2048
# ... and a background removal from this many patterns on (a block of the patterns per GPU, each over its own host link:
# a host-backed call is transfer-bound - patterns up, patterns down)
PREPROCESS_GROUP_MIN_POINTS = 16384


class DictionaryXmap:
    """Stand-in for the `xmap` of a dictionary signal: one rotation
    (unit quaternion) per dictionary pattern."""

    def __init__(self, rotations, phase_name=""):
        self.rotations = np.asarray(rotations, dtype=np.float64).reshape(-1, 4)
        self.phase_name = phase_name

    @classmethod
    def empty(cls, shape):
        """Like `CrystalMap.empty((n,))`: identity rotations."""
        shape = tuple(shape) if not isinstance(shape, int) else (shape,)
        q = np.zeros(shape + (4,))
        q[..., 0] = 1
        obj = cls(q.reshape(-1, 4))
        obj._shape = shape
        return obj

    @property
    def shape(self):
        return getattr(self, "_shape", (self.rotations.shape[0],))

    @property
    def size(self):
        return int(self.rotations.shape[0])


class _Axes:
    """See `EBSD.axes_manager`."""

    def __init__(self, navigation_shape, signal_shape):
        self.navigation_shape = tuple(int(v) for v in navigation_shape)
        self.signal_shape = tuple(int(v) for v in signal_shape)

    navigation_dimension = property(lambda self: len(self.navigation_shape))
    signal_dimension = property(lambda self: len(self.signal_shape))
    navigation_size = property(lambda self: int(np.prod(self.navigation_shape)) if self.navigation_shape else 0)
    signal_size = property(lambda self: int(np.prod(self.signal_shape)))

    def __repr__(self):
        return f"<axes: navigation {self.navigation_shape} | signal {self.signal_shape}>"


def reduction_axes(axis, navigation_dimension):
    """The array axes (sorted, each once) that `axis` of `EBSD.sum` / `mean` / `max` / `min` / `std` / `var` names on a
    signal with `navigation_dimension` navigation axes.  Axes count in HyperSpy's natural order - navigation axes first,
    then signal axes, each group in (x, y) order, the reverse of the array's: for (ny, nx, sy, sx) the indices 0, 1, 2, 3
    are the array axes 1, 0, 3, 2, so (0, 1) is the map and (2, 3) the detector; with one navigation axis (0 | 1, 2) is
    (x | dx, dy), with none (0, 1) is (dx, dy).  `axis`: an int (negative: from the end of that list), one of "x", "y",
    "dx", "dy", or a tuple / list of these; None: every navigation axis.  Anything else raises ValueError."""
    nd = int(navigation_dimension)
    order = list(range(nd))[::-1] + [nd + 1, nd]
    names = dict(zip(("x", "y")[:nd] + ("dx", "dy"), order))
    if axis is None:
        return tuple(range(nd))
    reduced = set()
    for ax in axis if isinstance(axis, (tuple, list)) else (axis,):
        if isinstance(ax, str) and ax in names:
            reduced.add(names[ax])
        elif isinstance(ax, numbers.Integral) and not isinstance(ax, bool) and -len(order) <= ax < len(order):
            reduced.add(order[ax])
        else:
            raise ValueError(f"axis {ax!r} is not an axis of a signal with {nd} navigation and 2 signal axes: an int in "
                             f"[{-len(order)}, {len(order)}) or one of {list(names)}")
    if not reduced:
        raise ValueError(f"axis {axis!r} names no axis")
    return tuple(sorted(reduced))


class ReducedSignal:
    """What an axis reduction of an `EBSD` signal leaves once a detector axis is gone (HyperSpy returns a `BaseSignal`
    there): `data` on the host - the kept axes in array order, shape (1,) when none is kept, as HyperSpy leaves one
    "Scalar" axis - `axes_manager` (shapes in HyperSpy's (x, y) order), `change_dtype` and `deepcopy`."""

    def __init__(self, data, navigation_shape=(), signal_shape=()):
        self.data = np.asarray(data)
        self._navigation_shape_rc = tuple(navigation_shape)
        self._signal_shape_rc = tuple(signal_shape)

    def __repr__(self):
        return f"<ReducedSignal, shape: {self.data.shape}, dtype: {self.data.dtype}>"

    @property
    def axes_manager(self):
        return _Axes(self._navigation_shape_rc[::-1], self._signal_shape_rc[::-1])

    def change_dtype(self, dtype):
        self.data = self.data.astype(dtype)

    def deepcopy(self):
        return ReducedSignal(np.array(self.data, copy=True), self._navigation_shape_rc, self._signal_shape_rc)


class VirtualBSEImage:
    """Virtual backscatter electron image(s) (signals/virtual_bse_image.py): `data`, the images in the last two axes
    (an RGB image: (ny, nx, 3), see `rgb_data`), and the three intensity methods of the reference's class, which run
    the stack functions of `kikuchipy_amd.pattern` with the images as the patterns."""

    def __init__(self, data, *, device=0):
        self.data = np.asarray(data)
        self._device = device

    def __repr__(self):
        return f"<VirtualBSEImage, shape: {self.data.shape}, dtype: {self.data.dtype}>"

    def deepcopy(self):
        return VirtualBSEImage(np.array(self.data, copy=True), device=self._device)

    @property
    def rgb_data(self):
        """An RGB image's `data` (ny, nx, 3) of uint8 / uint16 as HyperSpy's rgb8 / rgb16 dtype: (ny, nx) of fields R, G, B."""
        d = self.data
        if d.ndim < 1 or d.shape[-1] != 3 or d.dtype not in (np.dtype(np.uint8), np.dtype(np.uint16)):
            raise ValueError(f"data of shape {d.shape} and dtype {d.dtype} is not an RGB image")
        code = f"u{d.dtype.itemsize}"
        return np.ascontiguousarray(d).view([("R", code), ("G", code), ("B", code)])[..., 0]

    def _done(self, out, inplace):
        if inplace:
            self.data = out
            return None
        return VirtualBSEImage(out, device=self._device)

    def rescale_intensity(self, relative=False, in_range=None, out_range=None, dtype_out=None, percentiles=None,
                          show_progressbar=None, inplace=True, lazy_output=None):
        """signals/_kikuchipy_signal.py:88-243 through `kikuchipy_amd.pattern.rescale_intensity_stack`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        if in_range is not None and percentiles is not None:
            raise ValueError("'percentiles' must be None if 'in_range' is not None")
        elif relative is True and in_range is not None:
            raise ValueError("'in_range' must be None if 'relative' is True")
        out = _pattern.rescale_intensity_stack(self.data, in_range, out_range, dtype_out, percentiles,
                                               relative=bool(relative), device=self._device)
        return self._done(out, inplace)

    def normalize_intensity(self, num_std=1, divide_by_square_root=False, dtype_out=None, show_progressbar=None,
                            inplace=True, lazy_output=None):
        """signals/_kikuchipy_signal.py:245-338 through `kikuchipy_amd.pattern.normalize_intensity_stack`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        out = _pattern.normalize_intensity_stack(self.data, num_std, divide_by_square_root, dtype_out, device=self._device)
        return self._done(out, inplace)

    def adaptive_histogram_equalization(self, kernel_size=None, clip_limit=0.0, nbins=128, show_progressbar=None,
                                        inplace=True, lazy_output=None):
        """signals/_kikuchipy_signal.py:340-470 through `kikuchipy_amd.pattern.adaptive_histogram_equalization_stack`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        out = _pattern.adaptive_histogram_equalization_stack(self.data, kernel_size, clip_limit, nbins, device=self._device)
        return self._done(out, inplace)


class EBSD:
    def __init__(self, data, static_background=None, xmap=None, step_sizes=None, scan_unit="px",
                 device=None, devices=None, *, detector=None):
        """device: the GPU this signal's engine context lives on (None: GPU 0, and `dictionary_indexing`
        is free to shard the dictionary over every visible GPU); devices: "all" / a list of ids for
        `dictionary_indexing` (see `kikuchipy_amd.dictionary_indexing`); `detector`, `static_background`, `xmap`: the
        reference's custom attributes (signals/ebsd.py:188-199) - without a detector, one of the signal's shape."""
        self._resident = None  # the patterns in HBM (pattern._pattern.ResidentPatterns) once `to_device()` was called
        self.data = data
        self._detector = None
        ndim = data.ndim if hasattr(data, "ndim") else np.ndim(data)  # lazy data is not touched
        if ndim < 2 or ndim > 4:
            raise ValueError("EBSD data must have 0, 1 or 2 navigation axes and 2 signal axes")
        self._static_background = static_background  # (the constructor does not check: signals/ebsd.py:198-199)
        self._xmap = xmap
        self.step_sizes = step_sizes
        self.scan_unit = scan_unit
        self._device = device
        self._devices = devices
        self._ctx = None
        self._groups = {}  # device ids -> _lib.Group, kept from call to call (its communicator is made once)
        self._learning_results = None  # of the last `decomposition`; not carried over by `deepcopy` / `_like`
        if detector is not None:
            self.detector = detector

    @property
    def detector(self):
        """The detector - sample geometry (signals/ebsd.py:203-223): by default a detector of the signal's shape with
        the reference's default projection centre; setting one checks it against the signal as the reference does
        (signals/util/_detector.py:28-59)."""
        if self._detector is None:
            from kikuchipy_amd.detectors import EBSDDetector

            self._detector = EBSDDetector(shape=self._signal_shape_rc)
        return self._detector

    @property
    def xmap(self):
        """Crystal map of the signal (signals/ebsd.py:225-245): anything with a `shape`; setting one whose shape is not
        the navigation shape raises as the reference does (signals/util/_crystal_map.py:55-59)."""
        return self._xmap

    @xmap.setter
    def xmap(self, value):
        shape = getattr(value, "shape", None)
        nav = self._navigation_shape_rc
        if value is not None and shape is not None and tuple(shape) != nav and tuple(shape) != (nav or (1,)):
            raise ValueError(
                f"Crystal map shape {tuple(shape)} and signal's navigation shape {nav} must be the same "
                "(see EBSD.axes_manager)"
            )
        self._xmap = value

    @property
    def static_background(self):
        """Static background pattern (signals/ebsd.py:247-266); one of another data type or shape is set with the
        reference's warning (`remove_static_background` then refuses it)."""
        return self._static_background

    @static_background.setter
    def static_background(self, value):
        if value is not None:
            if getattr(value, "dtype", None) != self._data_dtype:
                warnings.warn("Background pattern has different data type from patterns")
            if tuple(getattr(value, "shape", ())) != self._signal_shape_rc:
                warnings.warn("Background pattern has different shape from patterns")
        self._static_background = value

    @detector.setter
    def detector(self, value):
        if tuple(value.shape) != self._signal_shape_rc:
            raise ValueError(f"Detector shape {value.shape} must be equal to the signal shape {self._signal_shape_rc}.")
        if value.navigation_shape != (1,) and value.navigation_shape != self._navigation_shape_rc:
            raise ValueError(
                "Detector must have exactly one projection center (PC), or one PC per pattern in an array of shape "
                "equal to signal's navigation shape + (3,)."
            )
        self._detector = value

    # ------------------------------------------------------------------ engines
    def close(self):
        """Destroy the engines this signal keeps from call to call (its own context, its groups over several GPUs -
        their host threads and communicators); they are made again when needed.  `with EBSD(...) as s:` calls it.  A
        resident signal brings its patterns to the host first."""
        self.to_host()  # (a resident signal's patterns would go with its context)
        for g in self._groups.values():
            g.close()
        self._groups = {}
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ where the patterns live
    @property
    def data(self):
        """The patterns as a host array.  On a resident signal the first read downloads them (after the recorded
        background steps) and the array is kept until the next method changes the patterns; assigning `data` makes the
        signal host-backed again."""
        if self._resident is not None and self._host is None:
            self._host = self._resident.host()
        return self._host

    @data.setter
    def data(self, value):
        self._host = value
        self._resident = None

    @property
    def is_resident(self):
        """Whether the patterns live in the HBM of this signal's context (`to_device`) or on the host (the default)."""
        return self._resident is not None

    def to_device(self):
        """Make the signal resident: one upload into this signal's engine context, which from now on owns the patterns -
        every method works on them there, nothing else uploads into that context.  Returns `self`."""
        if self._resident is None:
            if hasattr(self._host, "compute"):
                raise ValueError("lazy data cannot be made resident: compute it first")
            data = np.asarray(self._host)
            _pattern._upload(self.context, data)
            self._resident = _pattern.ResidentPatterns(self.context, data.shape[:-2])
            self._host = data  # (still what the device holds: kept as the host copy)
        return self

    def to_host(self):
        """Make the signal host-backed: one download, unless the host copy is current.  Returns `self`."""
        if self._resident is not None:
            self.data = self.data
        return self

    def _patterns_changed(self):
        """A method changed the resident patterns: the host copy is stale."""
        self._host = None

    @property
    def _data_shape(self):
        return tuple(self._resident.shape if self._resident is not None else self._host.shape)

    @property
    def _data_dtype(self):
        return self._resident.dtype if self._resident is not None else self._host.dtype

    def _own_device_only(self, devices, comm=None):
        """A resident signal works on the device that holds it: what a CALL names must be that device (the `devices`
        the signal was constructed with describe where a host-backed signal may spread, and are not consulted)."""
        own = self._device or 0
        ids = _lib.resolve_devices(devices)
        if comm is not None or (ids is not None and list(ids) != [own]):
            raise ValueError(f"a resident signal works on its own device ({own}): `devices` / `comm` cannot spread it over "
                             "others (multi-GPU residency is not implemented); call to_host() first")

    def _resident_twin(self, navigation_shape, fill):
        """A new resident signal on this signal's device with this one's custom attributes (deep copies), whose context
        `fill(context)` fills with patterns."""
        placeholder = np.broadcast_to(np.zeros((), dtype=self._data_dtype), tuple(navigation_shape) + (1, 1))
        out = EBSD(placeholder, None if self._static_background is None else np.array(self._static_background),
                   copy.deepcopy(self._xmap), self.step_sizes, self.scan_unit, self._device, self._devices)
        out._detector = None if self._detector is None else self._detector.deepcopy()
        if hasattr(self, "original_metadata"):
            out.original_metadata = self.original_metadata
        try:
            fill(out.context)
        except BaseException:
            out._discard()
            raise
        out._resident = _pattern.ResidentPatterns(out.context, navigation_shape)
        out._host = None
        return out

    def _discard(self):
        """Close this signal's engines without bringing anything back."""
        self._resident = None
        self.close()

    def _transform(self, inplace, devices, run):
        """What every pre-processing method ends with.  `run(patterns, engines)` calls the stack function with
        `**engines` (context / contexts).  Host-backed: upload, op, download; the result replaces `data` or goes into a
        new signal.  Resident: the op runs on the patterns where they are - of this signal (`inplace`), or of a
        device-to-device copy, which is returned."""
        if self._resident is not None:
            self._own_device_only(devices)
            target = self if inplace else self.deepcopy()
            try:
                run(target._resident.kept(), dict(context=target.context, contexts=None))
            except BaseException:
                if target is not self:
                    target._discard()
                raise
            target._patterns_changed()
            return None if inplace else target
        contexts = self._member_contexts(devices, PREPROCESS_GROUP_MIN_POINTS)
        out = run(np.asarray(self.data), dict(context=None if contexts else self.context, contexts=contexts))
        if inplace:
            self.data = out
            return None
        return self._like(out)

    def _read(self, devices, run, flat=False):
        """What every read-only method ends with: `run(patterns, engines)` on the host array or on the resident
        patterns (`flat`: as a stack of patterns)."""
        if self._resident is not None:
            self._own_device_only(devices)
            p = self._resident.flat() if flat else self._resident.kept(False)
            return run(p, dict(context=self.context, contexts=None))
        contexts = self._member_contexts(devices, PREPROCESS_GROUP_MIN_POINTS)
        data = np.asarray(self.data)
        if flat:
            data = data.reshape((-1,) + data.shape[-2:])
        return run(data, dict(context=None if contexts else self.context, contexts=contexts))

    # ------------------------------------------------------------------ shapes
    @property
    def _navigation_shape_rc(self):
        return self._data_shape[:-2]

    @property
    def _signal_shape_rc(self):
        return self._data_shape[-2:]

    @property
    def navigation_size(self):
        return int(np.prod(self._navigation_shape_rc)) if self._navigation_shape_rc else 0

    @property
    def axes_manager(self):
        """The four numbers scripts written for kikuchipy read from HyperSpy's axes manager around this path
        (`s.axes_manager.signal_shape[::-1]`, `sim.axes_manager.navigation_size // 10` in the reference's
        doc/tutorials/pattern_matching.ipynb): shapes in HyperSpy's (x, y) order - the REVERSE of the array's - and
        sizes.  Nothing else of the signal model is here (out of scope)."""
        return _Axes(self._navigation_shape_rc[::-1], self._signal_shape_rc[::-1])

    def deepcopy(self):
        """A copy that shares nothing with this signal; of a resident signal a resident one (a device-to-device copy
        into a context of its own)."""
        if self._resident is not None:
            src = self._resident
            return self._resident_twin(src.navigation_shape, lambda c: src.context.select_patterns(into=c))
        out = EBSD(np.array(self.data, copy=True),
                   None if self.static_background is None else np.array(self.static_background),
                   self.xmap, self.step_sizes, self.scan_unit, self._device, self._devices)
        out._detector = None if self._detector is None else self._detector.deepcopy()
        if hasattr(self, "original_metadata"):
            out.original_metadata = self.original_metadata
        return out

    @property
    def context(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self._device or 0)
        return self._ctx

    def _member_contexts(self, devices, min_points):
        """One engine context per GPU for work that splits over the map's points (pre-processing, refinement): the
        members of this signal's group over `devices` (or over every visible GPU when nothing was named and the map has
        `min_points` points or more), None = this signal's own context."""
        ids = _lib.resolve_devices(devices if devices is not None else self._devices)
        if ids is None and self._device is None and self.navigation_size >= min_points:
            ids = _lib.default_devices()
        if ids is None or len(ids) < 2:
            return None
        key = tuple(ids)
        if key not in self._groups:
            self._groups[key] = _lib.make_engine(devices=ids)
        return self._groups[key].members

    def _engine(self, devices, comm, dictionary_size):
        """The engine a `dictionary_indexing` call of this signal runs on: its own context, or a `Group`
        over several GPUs (kept on the signal from call to call)."""
        from kikuchipy_amd.indexing._dictionary_indexing import pick_devices

        device, ids = pick_devices(self._device, devices if devices is not None else self._devices, comm,
                                   max(self.navigation_size, 1), dictionary_size)
        if ids is not None and len(ids) == 1:
            device, ids = ids[0], None
        if ids is None:
            return device, (self.context if device == (self._device or 0) else _lib.Context(device))
        key = tuple(ids)
        if key not in self._groups:
            self._groups[key] = _lib.make_engine(devices=ids)
        return ids[0], self._groups[key]

    # ------------------------------------------------------------------ pre-processing
    def _like(self, data):
        """A new signal around `data` with this one's custom attributes (the reference carries `detector`,
        `static_background` and `xmap` over, signals/ebsd.py:564-573, :686-696)."""
        out = EBSD(data, self.static_background, self.xmap, self.step_sizes, self.scan_unit, self._device, self._devices)
        out._detector = None if self._detector is None else self._detector.deepcopy()
        if hasattr(self, "original_metadata"):
            out.original_metadata = self.original_metadata
        return out

    def remove_static_background(self, operation="subtract", static_bg=None, scale_bg=False, show_progressbar=None,
                                 inplace=True, lazy_output=None, *, devices=None):
        """signals/ebsd.py:442-573, with the reference's parameters in the reference's order.  `show_progressbar`
        is accepted and has nothing to show (the whole signal is one kernel launch per GPU); `lazy_output=True`
        (only with `inplace=False`, as there) returns an ordinary signal - the result is computed on the device either
        way, this package has no lazy experimental signal."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        if static_bg is None:
            static_bg = self.static_background
            if not isinstance(static_bg, np.ndarray) and not hasattr(static_bg, "compute"):
                raise ValueError("`EBSD.static_background` is not a valid array")
        return self._transform(inplace, devices, lambda p, engines: _pattern.remove_static_background(
            p, static_bg, operation, scale_bg, **engines))

    def remove_dynamic_background(self, operation="subtract", filter_domain="frequency", std=None, truncate=4.0,
                                  show_progressbar=None, inplace=True, lazy_output=None, *, devices=None):
        """signals/ebsd.py:575-696; `show_progressbar` / `lazy_output` as in `remove_static_background`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        return self._transform(inplace, devices, lambda p, engines: _pattern.remove_dynamic_background(
            p, operation, filter_domain, std, truncate, **engines))

    def fft_filter(self, transfer_function, function_domain, shift=False, show_progressbar=None, inplace=True,
                   lazy_output=None, *, devices=None):
        """signals/ebsd.py:805-930: filter every pattern in the frequency domain (`transfer_function` of the pattern
        shape, applied to the spectrum; `shift`: it is centred) or the spatial domain (a kernel, applied as Barnes' FFT
        convolution with edge-replicated borders), then rescale it to its dtype's range
        (`kikuchipy_amd.pattern.fft_filter_stack`); `show_progressbar` / `lazy_output` as in
        `remove_static_background`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        return self._transform(inplace, devices, lambda p, engines: _pattern.fft_filter_stack(
            p, transfer_function, function_domain, shift, **engines))

    def rescale_intensity(self, relative=False, in_range=None, out_range=None, dtype_out=None, percentiles=None,
                          show_progressbar=None, inplace=True, lazy_output=None, *, devices=None):
        """signals/_kikuchipy_signal.py:88-243: rescale every pattern onto `out_range` (default: the dtype range of
        `dtype_out`, which defaults to the data's dtype) from `in_range`, the global min / max (`relative`; NaN if any
        value is NaN), the per-pattern `percentiles` or the per-pattern min / max
        (`kikuchipy_amd.pattern.rescale_intensity_stack`).  With `inplace` `self.data` is replaced and may change its
        dtype; `show_progressbar` / `lazy_output` as in `remove_static_background`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        if in_range is not None and percentiles is not None:
            raise ValueError("'percentiles' must be None if 'in_range' is not None")
        elif relative is True and in_range is not None:
            raise ValueError("'in_range' must be None if 'relative' is True")
        _pattern.intensity_dtype_out(dtype_out, self._data_dtype)  # before any GPU work
        return self._transform(inplace, devices, lambda p, engines: _pattern.rescale_intensity_stack(
            p, in_range, out_range, dtype_out, percentiles, relative=bool(relative), **engines))

    def normalize_intensity(self, num_std=1, divide_by_square_root=False, dtype_out=None, show_progressbar=None,
                            inplace=True, lazy_output=None, *, devices=None):
        """signals/_kikuchipy_signal.py:245-338: `(p - mean) / (num_std * std [* sqrt(size)])` of every pattern as
        `dtype_out` (default: the data's dtype; `kikuchipy_amd.pattern.normalize_intensity_stack`); `inplace`,
        `show_progressbar` / `lazy_output` as in `rescale_intensity`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        _pattern.intensity_dtype_out(dtype_out, self._data_dtype)  # before any GPU work
        return self._transform(inplace, devices, lambda p, engines: _pattern.normalize_intensity_stack(
            p, num_std, divide_by_square_root, dtype_out, **engines))

    def adaptive_histogram_equalization(self, kernel_size=None, clip_limit=0.0, nbins=128, show_progressbar=None,
                                        inplace=True, lazy_output=None, *, devices=None):
        """signals/_kikuchipy_signal.py:340-470: scikit-image 0.18.3's equalize_adapthist of every pattern, then a
        rescale to the range of the data's dtype (`kikuchipy_amd.pattern.adaptive_histogram_equalization_stack`).
        `kernel_size` None gives (sx // 4, sy // 4) as (rows, cols), as the reference's HyperSpy order does; the
        reference's warnings for NaN and float data; `show_progressbar` / `lazy_output` as in
        `remove_static_background`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        # (float patterns of a resident signal: the checks below read the values - one lazy download, kept as the host
        # copy; integer patterns are not looked at)
        if self._resident is not None and self._data_dtype.kind != "f":
            data = self._resident.kept(False)
        else:
            data = np.asarray(self.data)
        if data.dtype.kind == "f" and np.isnan(data).any():
            warnings.warn("Equalization of signals with NaN data has been shown to give bad results")
        elif np.issubdtype(data.dtype, np.floating):
            warnings.warn(
                "Equalization of signals with floating point data type has been shown to give bad results. Rescaling "
                "intensities to integer intensities is recommended."
            )
        kernel_size = _pattern.clahe_kernel_size(kernel_size, self._signal_shape_rc)
        args = _pattern.clahe_arguments(data, kernel_size, clip_limit, nbins)  # before any GPU work
        if self._resident is not None:  # (checked above: the stack function would download the patterns to check again)
            return self._transform(inplace, devices, lambda p, engines: _pattern._process(
                p, lambda c: c.adaptive_histogram_equalization(*args), engines["context"], 0, None))
        return self._transform(inplace, devices, lambda p, engines: _pattern.adaptive_histogram_equalization_stack(
            p, kernel_size, clip_limit, nbins, **engines))

    def get_dynamic_background(self, filter_domain="frequency", std=None, truncate=4.0, dtype_out=None,
                               show_progressbar=None, lazy_output=None, *, devices=None, **kwargs):
        """signals/ebsd.py:698-803: the dynamic background of every pattern - the Gaussian blur that
        `remove_dynamic_background` removes - in a new signal of `dtype_out` (default: the data's dtype) with this
        one's custom attributes (`kikuchipy_amd.pattern.get_dynamic_background_stack`).  The reference hands `**kwargs`
        to its SciPy filter function; this engine has none, so any is refused.  `show_progressbar` / `lazy_output` as in
        `remove_static_background` (`lazy_output=True` returns an ordinary signal)."""
        if filter_domain not in ("frequency", "spatial"):
            raise ValueError(f"{filter_domain} must be either of ['frequency', 'spatial']")
        if kwargs:
            raise TypeError(f"get_dynamic_background() got keyword arguments {sorted(kwargs)} for the reference's SciPy "
                            "filter function, which this GPU engine does not call")
        _pattern.intensity_dtype_out(dtype_out, self._data_dtype)  # before any GPU work
        out = self._read(devices, lambda p, engines: _pattern.get_dynamic_background_stack(
            p, filter_domain, std, truncate, dtype_out, **engines))
        return self._like(out)

    def downsample(self, factor, dtype_out=None, show_progressbar=None, inplace=True, lazy_output=None, *,
                   devices=None):
        """signals/ebsd.py:1113-1219: bin every pattern by the integer `factor`, a divisor of both detector axes, and
        rescale it to the range of `dtype_out` (default: the data's dtype; `kikuchipy_amd.pattern.downsample_stack`).
        As in the reference the static background, if any, is binned and rescaled the same way into `dtype_out` (on
        the GPU, as a stack of one pattern), the detector becomes a copy with the new shape and `binning * factor`, and
        `xmap` carries over; with `inplace=False` this signal, its detector and its background stay untouched.
        `show_progressbar` / `lazy_output` as in `remove_static_background`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        factor = _pattern.check_binning_factor(factor, self._signal_shape_rc)
        dt = _pattern.intensity_dtype_out(dtype_out, self._data_dtype)  # before any GPU work
        static_bg = self.static_background
        if static_bg is not None:
            if hasattr(static_bg, "compute"):
                static_bg = static_bg.compute()
            # (a resident signal's context holds its patterns: the background is binned on a scratch context)
            static_bg = _pattern.downsample_stack(np.asarray(static_bg), factor, dt, device=self._device or 0,
                                                  context=None if self._resident is not None else self.context)
        detector = self.detector.deepcopy()  # (the default detector when none was set: the reference always has one)
        detector.shape = tuple(n // factor for n in self._signal_shape_rc)
        detector.binning = detector.binning * factor
        if self._resident is not None:
            out = self._transform(inplace, devices, lambda p, engines: _pattern.downsample_stack(p, factor, dt, **engines))
            out = self if inplace else out
        else:
            contexts = self._member_contexts(devices, PREPROCESS_GROUP_MIN_POINTS)
            data = _pattern.downsample_stack(np.asarray(self.data), factor, dt,
                                             context=None if contexts else self.context, contexts=contexts)
            out = self if inplace else EBSD(data, None, self.xmap, self.step_sizes, self.scan_unit, self._device,
                                            self._devices)
            out.data = data
        out._static_background = static_bg
        out._detector = detector
        out._learning_results = None  # (they belong to the patterns' old shape)
        if not inplace:
            if hasattr(self, "original_metadata"):
                out.original_metadata = self.original_metadata
            return out
        return None

    def change_dtype(self, dtype):
        """HyperSpy's `change_dtype` for the six pattern dtypes, in place: `ndarray.astype(dtype)` of every pattern on the
        GPU (kpdi_change_dtype: to integers by truncation with NumPy's wrap-around, to float32 by rounding).
        `static_background` is left alone.  The workflow's `change_dtype("float32")` before a decomposition and
        `change_dtype(dtype_orig)` after it."""
        dt = _pattern.intensity_dtype_out(dtype, self._data_dtype)
        if self._data_dtype.type not in _pattern.INTENSITY_DTYPES:
            raise ValueError(f"pattern dtype {self._data_dtype} is not supported by the GPU pre-processing kernels")
        if dt == self._data_dtype:
            return None
        if self._resident is not None:
            return self._transform(True, None, lambda p, engines: _pattern._process(
                p, lambda c: c.change_dtype(dt), engines["context"], 0, None))
        self.data = _pattern._process(np.asarray(self.data), lambda c: c.change_dtype(dt), self.context, 0, None)
        return None

    @property
    def learning_results(self):
        """The `kikuchipy_amd.pattern.LearningResults` of the last `decomposition`, None before one."""
        return self._learning_results

    def decomposition(self, normalize_poissonian_noise=False, algorithm="SVD", output_dimension=None, centre=None,
                      **kwargs):
        """HyperSpy's `decomposition` as the reference's multivariate-analysis workflow calls it: principal component
        analysis of the patterns, `s.decomposition(algorithm="SVD", output_dimension=100, centre="signal")`
        (`kikuchipy_amd.pattern.decomposition_stack`: a float64 Gram matrix and two products on the GPU, the
        eigen-solve in NumPy).  `centre`: None, "navigation" (subtract the mean pattern) or "signal" (subtract every
        pattern's mean intensity).  The results go to `learning_results`; the patterns stay as they are.  Only this form
        exists here: another `algorithm`, `normalize_poissonian_noise=True`, an `svd_solver` other than "auto" / "full"
        or any other keyword raises NotImplementedError before any GPU work.  Integer patterns raise TypeError as in
        HyperSpy: call `change_dtype("float32")` first."""
        if algorithm != "SVD":
            raise NotImplementedError(f"algorithm={algorithm!r}: only algorithm='SVD' is implemented")
        if normalize_poissonian_noise is not False:
            raise NotImplementedError(f"normalize_poissonian_noise={normalize_poissonian_noise!r}: only False is implemented")
        _decomposition.check_centre(centre)
        for name, value in kwargs.items():
            if name == "svd_solver" and value in ("auto", "full"):
                continue
            raise NotImplementedError(f"{name}={value!r} is not implemented by the GPU decomposition")
        checked = _decomposition.check_decomposition(self._data_shape, self._data_dtype, output_dimension, centre)
        patterns = np.asarray(self.data) if self._resident is None else self._resident.kept(False)
        self._learning_results = _decomposition._decompose(patterns, checked, centre, self.context)
        return None

    def get_decomposition_model(self, components=None, dtype_out="float32"):
        """signals/ebsd.py:2665-2723: the model signal rebuilt from `components` of the last decomposition - None: all,
        an int: the first `components`, a list of ints: those - as `_update_learning_results` picks them
        (signals/util/_dask.py:283-332): factors and loadings are cast to `dtype_out` (float32 / float64) first, then
        loadings factors^T plus the mean that centring removed is summed in float64 on the GPU and rounded once
        (`kikuchipy_amd.pattern.decomposition_model_stack`).  The new signal has this one's custom attributes and no
        learning results; this signal's stay as they are."""
        if self._learning_results is None:
            raise ValueError("No learning results found: run EBSD.decomposition() first")
        checked = _decomposition.check_model(self._data_shape, self._learning_results, components, dtype_out)
        if self._resident is not None:  # the model replaces the patterns of a device-to-device copy
            results = self._learning_results
            return self._transform(False, None, lambda p, engines: _decomposition._model(
                p, checked, results, dtype_out, engines["context"]))
        out = _decomposition._model(np.asarray(self.data), checked, self._learning_results, dtype_out, self.context)
        return self._like(out)

    def get_image_quality(self, normalize=True, show_progressbar=None, *, devices=None):
        """signals/ebsd.py:1312-1375: Q of every pattern (`kikuchipy_amd.pattern.get_image_quality` with the default
        frequency vectors), float32 of the navigation shape (0-d without navigation axes).  `show_progressbar` is
        accepted and has nothing to show."""
        q = self._read(devices, lambda p, engines: _pattern.get_image_quality(p, normalize, **engines), flat=True)
        return q.reshape(self._navigation_shape_rc)

    # ------------------------------------------------------------------ axis reductions
    def _reduce(self, op, axis, out, devices):
        """What `sum`, `mean`, `max`, `min`, `std` and `var` share (`kikuchipy_amd.pattern.reduce_stack`): the patterns
        are read where they are and only the result travels; this signal stays as it is, resident if it was.  The
        result is host-backed: an `EBSD` while both detector axes survive - `static_background` carried over, `xmap`
        dropped, the detector a deep copy, with the single PC `pc_average` once the navigation shape changed - else a
        `ReducedSignal`."""
        if out is not None:
            raise NotImplementedError("`out` is not implemented: the result is always a new, host-backed signal")
        nav, sig = self._navigation_shape_rc, self._signal_shape_rc
        if axis is None and not nav:
            return self
        axes = reduction_axes(axis, len(nav))
        if min(axes) >= len(nav):  # every pattern on its own: splits over GPUs like the other read-only ops
            data = self._read(devices, lambda p, engines: _pattern.reduce_stack(p, op, axes, **engines))
        elif self._resident is not None:
            self._own_device_only(devices)
            data = _pattern.reduce_stack(self._resident.kept(False), op, axes, context=self.context)
        else:
            ids = _lib.resolve_devices(devices)
            if ids is not None and len(ids) > 1:
                raise ValueError(f"a reduction over a navigation axis runs on one GPU, `devices` names {len(ids)}: partial "
                                 "results of several GPUs would be combined in another order")
            if ids is None or ids[0] == (self._device or 0):
                data = _pattern.reduce_stack(np.asarray(self.data), op, axes, context=self.context)
            else:
                data = _pattern.reduce_stack(np.asarray(self.data), op, axes, device=ids[0])
        nav_kept = tuple(n for k, n in enumerate(nav) if k not in axes)
        sig_kept = tuple(n for k, n in enumerate(sig, len(nav)) if k not in axes)
        if len(sig_kept) < 2:
            if not nav_kept and not sig_kept:
                return ReducedSignal(data.reshape(1), (), (1,))
            return ReducedSignal(data, nav_kept, sig_kept)
        result = EBSD(data, self.static_background, None, self.step_sizes, self.scan_unit, self._device, self._devices)
        if self._detector is not None:
            result._detector = self._detector.deepcopy()
            if nav_kept != nav:
                result._detector.pc = result._detector.pc_average
        if hasattr(self, "original_metadata"):
            result.original_metadata = self.original_metadata
        return result

    def sum(self, axis=None, out=None, rechunk=False, *, devices=None):
        """HyperSpy's `BaseSignal.sum` with its parameters in its order: the sum over `axis` (`reduction_axes`: ints in
        HyperSpy's order, "x", "y", "dx", "dy" or a tuple of these; None: every navigation axis) in NumPy's result
        dtype - uint64 / int64 for integer patterns, exact.  `out` other than None raises NotImplementedError, `rechunk`
        is accepted and ignored.  What comes back: `_reduce`."""
        return self._reduce("sum", axis, out, devices)

    def mean(self, axis=None, out=None, rechunk=False, *, devices=None):
        """`BaseSignal.mean`, as `sum`: float64 for integer patterns (NumPy's bits), else the patterns' dtype.
        `s.mean(axis=(0, 1))` is the mean pattern - the reference's static background when the vendor file has none -
        and `s.mean(axis=(2, 3))` the mean-intensity map."""
        return self._reduce("mean", axis, out, devices)

    def max(self, axis=None, out=None, rechunk=False, *, devices=None):
        """`BaseSignal.max`, as `sum`, in the patterns' dtype; NaN if one is met, as `np.max`."""
        return self._reduce("max", axis, out, devices)

    def min(self, axis=None, out=None, rechunk=False, *, devices=None):
        """`BaseSignal.min`, as `max`."""
        return self._reduce("min", axis, out, devices)

    def std(self, axis=None, out=None, rechunk=False, *, devices=None):
        """`BaseSignal.std`, as `mean` (no `ddof`: HyperSpy's takes none)."""
        return self._reduce("std", axis, out, devices)

    def var(self, axis=None, out=None, rechunk=False, *, devices=None):
        """`BaseSignal.var`, as `std`."""
        return self._reduce("var", axis, out, devices)

    def _region_sums(self, rects, devices=None):
        """`kikuchipy_amd.pattern.region_sums` of this signal's patterns: navigation shape + (n_rects,)."""
        return self._read(devices, lambda p, engines: _pattern.region_sums(p, rects, **engines))

    def get_virtual_bse_intensity(self, roi, out_signal_axes=None, *, devices=None):
        """signals/ebsd.py:1555-1598: the virtual backscatter electron image formed by the intensity within `roi` on the
        detector, `np.nansum` of every pattern over it: a `VirtualBSEImage` of the navigation shape, uint64 / int64 for
        integer patterns as NumPy's sum.  `roi`: anything with `left`, `top`, `right` and `bottom`
        (`kikuchipy_amd.imaging.RectangularROI`, `roi_to_rect`).  `out_signal_axes`: None, or the first navigation axes
        in HyperSpy's order in the order the image shall have them: (1, 0) transposes."""
        from kikuchipy_amd import imaging

        nav = self._navigation_shape_rc
        if out_signal_axes is None:
            out_signal_axes = list(range(min(len(nav), 2)))
        out_signal_axes = list(out_signal_axes)
        if len(out_signal_axes) > len(nav):
            raise ValueError("The length of 'out_signal_axes' cannot be longer than the navigation dimension of the signal")
        if sorted(out_signal_axes) != list(range(len(out_signal_axes))):
            raise ValueError(f"out_signal_axes {out_signal_axes} is not a permutation of the first navigation axes")
        rect = imaging.roi_to_rect(roi, self._signal_shape_rc, imaging.signal_axes(self))
        image = self._region_sums([rect], devices)[..., 0]
        if out_signal_axes == [1, 0]:
            image = np.ascontiguousarray(image.T)
        return VirtualBSEImage(image)

    def average_neighbour_patterns(self, window="circular", window_shape=(3, 3), show_progressbar=None, inplace=True,
                                   lazy_output=None, *, devices=None, **kwargs):
        """signals/ebsd.py:943-1111: average every pattern with its neighbours in the map under `window` (a valid
        `filters.Window`, or what `Window(window=window, shape=window_shape, **kwargs)` makes), divide by the point's
        truncated window sum and rescale to the dtype's range (`kikuchipy_amd.pattern.average_neighbour_patterns_stack`).
        A window of shape (1,) or (1, 1) warns and does nothing; a 1-D window on a 2-D map acts along the first
        navigation axis of the array; `show_progressbar` / `lazy_output` as in `remove_static_background`."""
        if lazy_output and inplace:
            raise ValueError("'lazy_output=True' requires 'inplace=False'")
        win = _neighbours.averaging_window(window, window_shape, **kwargs)
        if win.shape in [(1,), (1, 1)]:
            warnings.warn(f"A window of shape {win.shape} was passed, no averaging is therefore performed")
            return None
        nav = self._navigation_shape_rc
        w = _neighbours.window_on_map(win, nav)  # before any GPU work, as the window sums the stack function checks
        if not _neighbours.neighbour_window_sums(w, nav[0], nav[1] if len(nav) == 2 else 1).all():
            raise ValueError("The window sum of a map point is 0: its average is undefined")
        return self._transform(inplace, devices, lambda p, engines: _neighbours.average_neighbour_patterns_stack(
            p, win, **engines))

    def get_neighbour_dot_product_matrices(self, window=None, zero_mean=True, normalize=True, dtype_out="float32",
                                           show_progressbar=None, *, devices=None):
        """signals/ebsd.py:1221-1310: per map point the dot products of its pattern with the neighbours `window`
        selects (None: the nearest ones, `Window("circular", (3, 3)[:nav_dim])`), an array of the navigation shape +
        the window's shape (`kikuchipy_amd.pattern.neighbour_dot_product_matrices`).  `show_progressbar` is accepted
        and has nothing to show."""
        nav = self._navigation_shape_rc
        window = _neighbours.dot_product_window(window, nav)  # before any GPU work
        _neighbours._dot_dtype(dtype_out)
        return self._read(devices, lambda p, engines: _neighbours.neighbour_dot_product_matrices(
            p, window, zero_mean, normalize, dtype_out, **engines))

    def get_average_neighbour_dot_product_map(self, window=None, zero_mean=True, normalize=True, dtype_out="float32",
                                              dp_matrices=None, show_progressbar=None, *, devices=None):
        """signals/ebsd.py:1377-1491: the average dot product (ADP) map, per map point the mean of the dot products with
        its neighbours (`kikuchipy_amd.pattern.average_neighbour_dot_product_map`); with `dp_matrices` (of
        `get_neighbour_dot_product_matrices` and the same `window`) it is their mean, taken on the host."""
        nav = self._navigation_shape_rc
        window = _neighbours.dot_product_window(window, nav)  # before any GPU work
        if dp_matrices is not None:
            return _neighbours.average_dot_product_map_from_matrices(dp_matrices, window, len(nav))
        _neighbours._dot_dtype(dtype_out)
        return self._read(devices, lambda p, engines: _neighbours.average_neighbour_dot_product_map(
            p, window, zero_mean, normalize, dtype_out, **engines))

    # ------------------------------------------------------------------ selecting data
    @property
    def inav(self):
        """`s.inav[x, y]`: a new signal of the chosen map points, in HyperSpy's (x, y) order - `s.inav[:, 0]` is the
        first map row.  Integers (which drop their axis), slices with positive steps, negative indices as NumPy reads
        them; float indices (HyperSpy's indexing by axis value) are not implemented and raise.  `xmap`, per-point PCs
        and `step_sizes` follow (signals/ebsd.py:2830-2876, :3294-3377)."""
        return _Slicer(self, True)

    @property
    def isig(self):
        """`s.isig[x, y]`: a new signal of the chosen detector pixels, in HyperSpy's (x, y) order -
        `s.isig[5:55, 10:50]` is columns 5:55 and rows 10:50.  Slices only (an integer would remove a signal axis).
        `static_background` is sliced and the detector cropped (`EBSDDetector.crop`)."""
        return _Slicer(self, False)

    def crop(self, axis, start=None, end=None, convert_units=False):
        """Crop the signal in place along `axis` to [start, end): an int into the axes in HyperSpy's order - navigation
        (x, y), then signal (dx, dy) - or one of those names (signals/ebsd.py:2726-2770).  `crop(2, 5, 55)` then
        `crop("dy", 10, 50)` equals `isig[5:55, 10:50]`."""
        if convert_units:
            raise NotImplementedError("convert_units=True is not implemented: this signal's axes carry no units to convert")
        nav_dim = len(self._navigation_shape_rc)
        kind, i = _selection.crop_axis(axis, nav_dim)
        key = [slice(None)] * (nav_dim if kind == "navigation" else 2)
        key[i] = slice(start, end)
        self._select(tuple(key), kind == "navigation", inplace=True)

    def crop_signal(self, top=None, bottom=None, left=None, right=None, convert_units=False):
        """Crop the patterns in place to rows [top, bottom) and columns [left, right) (HyperSpy's
        `Signal2D.crop_signal`, which calls `crop` per axis)."""
        if convert_units:
            raise NotImplementedError("convert_units=True is not implemented: this signal's axes carry no units to convert")
        self._select((slice(left, right), slice(top, bottom)), False, inplace=True)

    def extract_grid(self, grid_shape, return_indices=False):
        """signals/ebsd.py:267-378: a new signal with the patterns at the points of a grid of `grid_shape` - an int, or
        (n columns, n rows) - evenly spaced in the map (`kikuchipy_amd._selection.grid_indices`); with
        `return_indices` also their indices into `data`, an array of shape (2,) + the grid's shape (rows first).  The
        detector's per-point PCs are picked at the grid points, `step_sizes` are scaled by the spacing, `xmap` is
        indexed if it supports it."""
        if isinstance(grid_shape, (int, np.integer)):
            grid_shape = (int(grid_shape),)
        grid_shape = tuple(grid_shape)
        nav_xy = self._navigation_shape_rc[::-1]
        if len(grid_shape) != len(nav_xy) or any(g > n for g, n in zip(grid_shape, nav_xy)):
            raise ValueError(f"grid_shape {grid_shape} must be compatible with navigation shape {nav_xy}")
        nav = self._navigation_shape_rc
        idx, spacing = _selection.grid_indices(grid_shape[::-1], nav, return_spacing=True)
        flat = np.ascontiguousarray((idx[0] * nav[1] + idx[1] if len(nav) == 2 else idx[0]).ravel(), dtype=np.int64)
        new_nav = tuple(idx.shape[1:])
        new = self._selected(flat, new_nav, None, None, inplace=False)
        try:
            mask = np.zeros(nav, dtype=bool)
            mask[tuple(idx)] = True
            new._xmap = None if self._xmap is None else self._xmap[mask.ravel()].deepcopy()
        except (IndexError, TypeError, ValueError, AttributeError):
            new._xmap = None
        det = self.detector.deepcopy()
        if det.navigation_shape == nav:
            det.pc = det.pc[tuple(idx)]
        elif det.navigation_shape != (1,):
            det.pc = [0.5, 0.5, 0.5]
        new._detector = det
        if self.step_sizes is not None and len(self.step_sizes) == len(nav):
            new.step_sizes = tuple(s * int(sp) for s, sp in zip(self.step_sizes, spacing))
        return (new, idx) if return_indices else new

    def _select(self, key, is_navigation, inplace=False):
        """`inav[key]` / `isig[key]` (a new signal) or, `inplace`, the same selection on this signal."""
        nav, sig = self._navigation_shape_rc, self._signal_shape_rc
        if is_navigation:
            flat, new_nav, axes = _selection.navigation_selection(nav, key)
            out = self._selected(flat, new_nav, None, None, inplace)
            # the reference's _update_custom_attributes (signals/ebsd.py:3352-3375), in array order
            slices = tuple(f if dropped else slice(f, f + s * (c - 1) + 1, s) for f, s, c, dropped in axes)
            try:
                out._xmap = None if self._xmap is None else self._xmap[slices]
            except (IndexError, TypeError, ValueError, AttributeError):
                out._xmap = None
            det = out._detector
            if det is not None and det.navigation_shape != (1,):
                pc = det.pc[slices] if det.navigation_shape == nav else np.empty(0)
                det.pc = pc if pc.size else [0.5, 0.5, 0.5]
            if self.step_sizes is not None and len(self.step_sizes) == len(nav):
                out.step_sizes = tuple(size * s for size, (_, s, _, dropped) in zip(self.step_sizes, axes) if not dropped)
            return None if inplace else out
        rows, cols = _selection.signal_selection(sig, key)
        old_detector = self.detector.deepcopy()
        out = self._selected(None, nav, rows, cols, inplace)
        rs, cs = (slice(f, f + s * (c - 1) + 1, s) for f, s, c in (rows, cols))
        bg = self._static_background
        if bg is not None:
            try:
                out._static_background = np.ascontiguousarray(bg[rs, cs])
            except (TypeError, IndexError):
                pass  # (as the reference: a background that cannot be sliced stays)
        try:
            if rows[1] != 1 or cols[1] != 1:
                raise ValueError("a detector is cropped to a rectangle of adjacent pixels")
            out._detector = old_detector.crop((rows[0], rows[0] + rows[2], cols[0], cols[0] + cols[2]))
        except ValueError:
            from kikuchipy_amd.detectors import EBSDDetector

            out._detector = EBSDDetector(shape=(rows[2], cols[2]), pc=[0.5, 0.5, 0.5], sample_tilt=old_detector.sample_tilt,
                                         tilt=old_detector.tilt, azimuthal=old_detector.azimuthal,
                                         px_size=old_detector.px_size, binning=old_detector.binning)
        return None if inplace else out

    def _selected(self, flat, new_nav, rows, cols, inplace):
        """The data of a selection - patterns `flat` (indices into the flattened map, None: all) in the navigation shape
        `new_nav`, detector rows / columns (first, step, count) (None: all) - as a new signal with deep copies of this
        one's attributes, or in this signal.  Host-backed: NumPy indexing into a contiguous copy.  Resident:
        kpdi_select_patterns, in place or into the new signal's context."""
        sy, sx = self._signal_shape_rc
        rows = (0, 1, sy) if rows is None else rows
        cols = (0, 1, sx) if cols is None else cols
        if self._resident is not None:
            src = self._resident
            _pattern._upload(src.context, src)  # (a signal mask left by an indexing run goes: the shape may change)
            if inplace:
                src.context.select_patterns(flat, rows, cols)
                self._resident = _pattern.ResidentPatterns(src.context, new_nav)
                self._patterns_changed()
                out = self
            else:
                out = self._resident_twin(new_nav, lambda c: src.context.select_patterns(flat, rows, cols, into=c))
        else:
            data = np.asarray(self.data)
            stack = data.reshape((-1, sy, sx))
            if flat is not None:
                stack = stack[flat]
            rs, cs = (slice(f, f + s * (c - 1) + 1, s) for f, s, c in (rows, cols))
            picked = np.ascontiguousarray(stack[:, rs, cs]).reshape(tuple(new_nav) + (rows[2], cols[2]))
            if np.may_share_memory(picked, data):
                picked = picked.copy()
            if inplace:
                self.data = picked
                out = self
            else:
                out = EBSD(picked, None if self._static_background is None else np.array(self._static_background),
                           copy.deepcopy(self._xmap), self.step_sizes, self.scan_unit, self._device, self._devices)
                out._detector = None if self._detector is None else self._detector.deepcopy()
                if hasattr(self, "original_metadata"):
                    out.original_metadata = self.original_metadata
        out._learning_results = None  # (they belong to the data's old shape)
        return out

    # ------------------------------------------------------------------ refinement
    def _refine(self, mode, xmap, detector, master_pattern, energy, navigation_mask, signal_mask,
                pseudo_symmetry_ops, method, method_kwargs, trust_region, initial_step, rtol, maxeval, compute,
                verbose, comm=None, devices=None):
        from kikuchipy_amd.indexing._refinement import refine

        # the points are independent: with several GPUs (named, or all of them for a map worth it) each refines a block
        contexts = self._member_contexts(devices, REFINE_GROUP_MIN_POINTS) if comm is None else None
        return refine(mode, np.asarray(self.data), _rotations_of(xmap), detector, master_pattern, energy,
                      navigation_mask, signal_mask, pseudo_symmetry_ops, method, method_kwargs, trust_region,
                      initial_step, rtol, maxeval, context=None if contexts else self.context, verbose=verbose, comm=comm,
                      compute=compute, contexts=contexts, is_in_data=getattr(xmap, "is_in_data", None),
                      xmap_shape=getattr(xmap, "shape", None) if hasattr(xmap, "is_in_data") else None)

    def refine_orientation(self, xmap, detector, master_pattern, energy=None, navigation_mask=None,
                           signal_mask=None, pseudo_symmetry_ops=None, method="minimize", method_kwargs=None,
                           trust_region=None, initial_step=None, rtol=1e-4, maxeval=None, compute=True,
                           rechunk=True, chunk_kwargs=None, *, verbose=True, comm=None, devices=None):
        """signals/ebsd.py:1986-2185.  `xmap`: anything with `.rotations`
        (e.g. the result of `dictionary_indexing`) or a quaternion array.
        Returns a `RefinementResult` (`rotations`, `scores`, `num_evals`,
        `pseudo_symmetry_index`); with `compute=False` a `DeferredRefinement`, finished by
        `kikuchipy_amd.indexing.compute_refine_orientation_results` (the reference: a lazy Dask array)."""
        out = self._refine("ori", xmap, detector, master_pattern, energy, navigation_mask, signal_mask,
                           pseudo_symmetry_ops, method, method_kwargs, trust_region, initial_step, rtol, maxeval,
                           compute, verbose, comm, devices)
        return out[0] if compute else out  # compute=False: a DeferredRefinement (compute_refine_orientation_results)

    def refine_projection_center(self, xmap, detector, master_pattern, energy=None, navigation_mask=None,
                                 signal_mask=None, method="minimize", method_kwargs=None, trust_region=None,
                                 initial_step=None, rtol=1e-4, maxeval=None, compute=True, rechunk=True,
                                 chunk_kwargs=None, *, verbose=True, comm=None, devices=None):
        """signals/ebsd.py:2187-2390.  Returns `(scores, new_detector, num_evals)`
        like the reference."""
        out = self._refine("pc", xmap, detector, master_pattern, energy, navigation_mask, signal_mask, None,
                           method, method_kwargs, trust_region, initial_step, rtol, maxeval, compute, verbose, comm, devices)
        if not compute:
            return out  # a DeferredRefinement (compute_refine_projection_center_results)
        res, det = out
        return res.scores, det, res.num_evals

    def refine_orientation_projection_center(self, xmap, detector, master_pattern, energy=None,
                                             navigation_mask=None, signal_mask=None, pseudo_symmetry_ops=None,
                                             method="minimize", method_kwargs=None, trust_region=None,
                                             initial_step=None, rtol=1e-4, maxeval=None, compute=True,
                                             rechunk=True, chunk_kwargs=None, *, verbose=True, comm=None, devices=None):
        """signals/ebsd.py:2392-2700.  Returns `(RefinementResult, new_detector)`."""
        return self._refine("ori_pc", xmap, detector, master_pattern, energy, navigation_mask, signal_mask,
                            pseudo_symmetry_ops, method, method_kwargs, trust_region, initial_step, rtol, maxeval,
                            compute, verbose, comm, devices)

    # ------------------------------------------------------------------ indexing
    def hough_indexing(self, phase_list, indexer, chunksize=528, verbose=1, return_index_data=False, return_band_data=False):
        """signals/ebsd.py:1600-1719: index the patterns - where they are, resident or on the host - by Hough indexing
        with an indexer of `EBSDDetector.get_indexer` (kikuchipy_amd/indexing/_hough_indexing.py; this package's own
        algorithm, not PyEBSDIndex's).  Returns a `HoughIndexingResult` (`rotations`, `fit`, `cm`, `pq`, `nmatch`,
        `phase_id` with -1 where not indexed, `is_in_data`) and on request `index_data` (n_phases + 1, M) and `band_data`
        (M, nBands)."""
        from kikuchipy_amd.indexing import _hough_indexing

        return _hough_indexing.hough_indexing(self, phase_list, indexer, chunksize, verbose, return_index_data, return_band_data)

    def hough_indexing_optimize_pc(self, pc0, indexer, batch=False, method="Nelder-Mead", **kwargs):
        """signals/ebsd.py:1721-1825: a detector with the PC (`batch=True`: one per pattern, in the navigation shape)
        that minimises the mean `fit` of Hough indexing, found by a Nelder-Mead search from `pc0` that detects the bands
        once and runs only the indexing per step: with `batch` and plain `options` (xatol, fatol, maxiter, maxfev) all
        searches on the device, one lane per pattern, else SciPy's on the host with one kernel
        launch per step - the same bits either way.  `method="PSO"` is not implemented."""
        from kikuchipy_amd.indexing import _hough_indexing

        return _hough_indexing.hough_indexing_optimize_pc(self, pc0, indexer, batch, method, **kwargs)

    def dictionary_indexing(self, dictionary, metric="ncc", keep_n=20, n_per_iteration=None,
                            navigation_mask=None, signal_mask=None, rechunk=False, dtype=None, *,
                            devices=None, comm=None, verbose=True, compute=None):
        """See `kikuchipy_amd.dictionary_indexing`; `dictionary` is an `EBSD`
        with a 1-D navigation axis and an `xmap` of equal size.  As there, a call that names no
        device shards the dictionary over every visible GPU from this one process.  A resident signal
        (`to_device`) is matched where it is, without an upload, on its own device: naming other
        `devices`, or a `comm`, raises a ValueError, and so does a `ResidentDictionary` (it lives in an
        engine of its own: `to_host()` first)."""
        from kikuchipy_amd.indexing._resident_dictionary import ResidentDictionary

        if self._resident is not None:
            self._own_device_only(devices, comm)
        if isinstance(dictionary, ResidentDictionary):
            if self._resident is not None:
                # the dictionary lives in its own engine, the patterns in this signal's: matching them would take a
                # silent download and an upload of the whole set
                raise ValueError("a resident signal cannot be indexed against a ResidentDictionary, which keeps its "
                                 "patterns in an engine of its own: call to_host() first (one download), or index "
                                 "against the dictionary signal itself")
            # prepared once and kept in HBM: only the match runs (metric and signal mask are its own)
            if tuple(dictionary.shape[1:]) != self._signal_shape_rc:
                raise ValueError(
                    f"Experimental {self._signal_shape_rc} and dictionary {tuple(dictionary.shape[1:])} signal "
                    "shapes must be identical"
                )
            return _dictionary_indexing(
                self.data, dictionary, metric, keep_n, n_per_iteration, navigation_mask, signal_mask, rechunk,
                dtype, step_sizes=self.step_sizes, scan_unit=self.scan_unit, device=self._device, comm=comm,
                compute=compute, verbose=verbose,
            )
        dict_data = dictionary.data
        dict_nav = dictionary._navigation_shape_rc
        dict_size = int(np.prod(dict_nav)) if dict_nav else 0
        dict_xmap = dictionary.xmap
        sig_exp, sig_dict = self._signal_shape_rc, dictionary._signal_shape_rc
        if sig_exp != sig_dict:
            raise ValueError(
                f"Experimental {sig_exp} and dictionary {sig_dict} signal shapes must be identical"
            )
        if dict_xmap is None or dict_xmap.shape != (dict_size,) or len(dict_nav) != 1:
            raise ValueError(
                "Dictionary signal must have a non-empty `EBSD.xmap` attribute of equal"
                " size as the number of dictionary patterns, and both the signal and "
                "crystal map must have only one navigation dimension"
            )
        from kikuchipy_amd.indexing.similarity_metrics import METRICS

        if isinstance(metric, str) and metric in METRICS:
            # on this signal's engine (one context, or a group over several GPUs): its device buffers - and a group's
            # communicator - are reused from call to call
            if self._resident is not None:  # on the context that holds the patterns, and nowhere else
                device, engine = self._device or 0, self.context
            else:
                device, engine = self._engine(devices, comm, dict_size)
            metric = METRICS[metric](device=device, compute=compute, context=engine)
            metric.rechunk = rechunk
        res = _dictionary_indexing(
            self.data if self._resident is None else self._resident.kept(False), dict_data, metric, keep_n,
            n_per_iteration, navigation_mask, signal_mask, rechunk, dtype, step_sizes=self.step_sizes, dictionary_rotations=dict_xmap.rotations,
            phase_name=getattr(dict_xmap, "phase_name", None), scan_unit=self.scan_unit, device=self._device, comm=comm,
            compute=compute,
            verbose=verbose,
        )
        # the phase list the reference hands to the returned CrystalMap (indexing/_dictionary_indexing.py:165): kept for
        # `to_crystal_map()` when the dictionary's crystal map is orix's
        res.phase_list = getattr(dict_xmap, "phases_in_data", None)
        return res


class _Slicer:
    """`EBSD.inav` / `EBSD.isig`: indexing returns a new signal."""

    def __init__(self, signal, is_navigation):
        self._signal = signal
        self._is_navigation = is_navigation

    def __getitem__(self, key):
        return self._signal._select(key, self._is_navigation)


def _rotations_of(xmap):
    """Quaternions of an indexing result / crystal-map-like object / plain array."""
    rot = getattr(xmap, "rotations", xmap)
    return np.asarray(getattr(rot, "data", rot), dtype=np.float64)


def _lambert2vector(x, y):
    """Square Lambert (X, Y) to vectors (n, 3), `_lambert2vector` of signals/util/_master_pattern.py:717-760 with the
    same operations on whole arrays (not normalised, as there)."""
    xi = x * np.sqrt(np.pi / 2)
    yi = y * np.sqrt(np.pi / 2)
    cart = np.zeros((x.size, 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        qy = 2 * yi * np.sqrt(np.pi - yi**2) / np.pi
        qqy = xi * np.pi * 0.25 / yi
        qx = 2 * xi * np.sqrt(np.pi - xi**2) / np.pi
        qqx = yi * np.pi * 0.25 / xi
        by_y = np.stack([qy * np.sin(qqy), qy * np.cos(qqy), 1 - 2 * yi**2 / np.pi], axis=1)
        by_x = np.stack([qx * np.cos(qqx), qx * np.sin(qqx), 1 - 2 * xi**2 / np.pi], axis=1)
    use_y = np.abs(xi) <= np.abs(yi)
    cart[use_y] = by_y[use_y]
    cart[~use_y] = by_x[~use_y]
    cart[np.maximum(np.abs(xi), np.abs(yi)) == 0] = [0, 0, 1]
    return cart


class EBSDMasterPattern:
    """Master pattern in the square Lambert projection: the surface of
    `kikuchipy.signals.EBSDMasterPattern` that `get_patterns` reads.

    Parameters
    ----------
    data
        (npy, npx), (2, npy, npx) [hemisphere], (n_energies, npy, npx) [energy]
        or (2, n_energies, npy, npx) [hemisphere, energy], as HyperSpy orders the
        reference's navigation axes.
    projection
        Must be "lambert" for `get_patterns` (as in the reference).
    hemisphere
        "upper", "lower" or "both"; "both" needs the leading axis of size 2.
    energies
        Energy axis values in kV when `data` has an energy axis.
    has_inversion_symmetry
        Whether the phase's point group contains inversion
        (`phase.point_group.contains_inversion`; orix is not a dependency here).
        `None` = no valid point group.
    """

    def __init__(self, data, projection="lambert", hemisphere=None, energies=None, phase_name="",
                 has_inversion_symmetry=True, device=0):
        self.data = np.asarray(data)
        if self.data.ndim < 2 or self.data.ndim > 4:
            raise ValueError("master pattern data must have 2 signal axes and at most 2 navigation axes")
        # (_utils/vector.py:47-60, _utils/exceptions.py:21-36: case-insensitive, the reference's texts)
        if not isinstance(projection, str) or projection.lower() not in ("stereographic", "lambert"):
            raise ValueError(f"Unknown projection {projection!r}, options are 'stereographic' and 'lambert'")
        self.projection = projection.lower()
        self.energies = None if energies is None else np.asarray(energies, dtype=np.float64)
        n_nav = self.data.ndim - 2
        has_energy = self.energies is not None
        if hemisphere is None:
            hemisphere = "both" if n_nav - int(has_energy) == 1 else "upper"
        if not isinstance(hemisphere, str) or hemisphere.lower() not in ("upper", "lower", "both"):
            raise ValueError(f"Unknown hemisphere {hemisphere!r}, options are 'upper', 'lower', or 'both'")
        hemisphere = hemisphere.lower()
        self.hemisphere = hemisphere
        expected_nav = int(hemisphere == "both") + int(has_energy)
        if expected_nav != n_nav or (hemisphere == "both" and self.data.shape[0] != 2):
            raise ValueError(
                f"data of shape {self.data.shape} does not match hemisphere='{hemisphere}' and "
                f"{'an' if has_energy else 'no'} energy axis"
            )
        if has_energy and self.data.shape[n_nav - 1] != self.energies.size:
            raise ValueError("`energies` must have one value per master pattern along the energy axis")
        self.phase_name = phase_name
        self.has_inversion_symmetry = has_inversion_symmetry
        self._device = device

    @property
    def _has_multiple_energies(self):
        return self.energies is not None

    # signals/ebsd_master_pattern.py:331-377
    def _is_suitable_for_projection(self, raise_if_not=False):
        error = None
        if self.projection != "lambert":
            error = NotImplementedError("Master pattern must be in the square Lambert projection")
        if self.has_inversion_symmetry is None:
            error = AttributeError("Master pattern `phase` attribute must have a valid point group")
        elif self.hemisphere != "both" and not self.has_inversion_symmetry:
            error = AttributeError(
                "For point groups without inversion symmetry, both hemispheres must be present in the "
                "master pattern signal"
            )
        if error is not None and raise_if_not:
            raise error
        return error is None

    def deepcopy(self):
        """A copy that shares nothing with this master pattern."""
        return copy.deepcopy(self)

    # signals/_kikuchi_master_pattern.py:135-213
    def as_lambert(self, show_progressbar=None):
        """Return a new master pattern in the Lambert projection: the same data shape in float32, every navigation
        slice (hemisphere, energy) interpolated from the stereographic one with the reference's steps (the Lambert grid,
        its unit vectors, their stereographic coordinates, `scipy.interpolate.interpn(method="splinef2d")`).  Runs on the
        host, once per master pattern; `show_progressbar` is accepted for the reference's signature."""
        if self.projection == "lambert":
            warnings.warn("Already in the Lambert projection, returning a deepcopy", UserWarning)
            return self.deepcopy()
        try:
            from scipy.interpolate import interpn
        except ImportError as e:  # pragma: no cover
            raise ImportError("EBSDMasterPattern.as_lambert needs SciPy (scipy.interpolate.interpn fits the spline)") from e

        sig_shape = self.data.shape[-2:]
        arr = np.linspace(-1, 1, sig_shape[0], dtype=np.float64)
        x_lambert, y_lambert = np.meshgrid(arr, arr)
        xyz_upper = _lambert2vector(x_lambert.ravel(), y_lambert.ravel())
        # orix' StereographicProjection().vector2xy (pole -1): (x, y) / (1 + z)
        x_stereo = xyz_upper[:, 0] / (1 + xyz_upper[:, 2])
        y_stereo = xyz_upper[:, 1] / (1 + xyz_upper[:, 2])
        x_stereo += 1
        y_stereo += 1
        kwargs = {"points": (arr + 1, arr + 1), "xi": (y_stereo, x_stereo), "method": "splinef2d"}
        data_out = np.zeros(self.data.shape, dtype=np.float32)
        for idx in np.ndindex(self.data.shape[:-2]):
            data_i = interpn(values=self.data[idx], **kwargs)
            data_out[idx] = data_i.reshape(sig_shape)
        return self.__class__(data_out, projection="lambert", hemisphere=copy.deepcopy(self.hemisphere),
                              energies=None if self.energies is None else self.energies.copy(), phase_name=self.phase_name,
                              has_inversion_symmetry=self.has_inversion_symmetry, device=self._device)

    # signals/_kikuchi_master_pattern.py:303-345
    def _get_master_pattern_arrays_from_energy(self, energy=None):
        data = self.data
        if self._has_multiple_energies:
            if energy is None:
                energy = self.energies[-1]
            # HyperSpy float indexing (`inav[float]`): the axis value closest to `energy`
            idx = int(np.argmin(np.abs(self.energies - float(energy))))
            data = data[:, idx] if self.hemisphere == "both" else data[idx]
        if self.hemisphere == "both":
            return data[0], data[1]
        return data, data

    def get_patterns(self, rotations, detector, energy=None, dtype_out="float32", compute=False,
                     show_progressbar=None, **kwargs):
        """Patterns projected onto `detector`, one per rotation.

        `rotations`: (..., 4) unit quaternions (a, b, c, d) with at most two
        leading axes (an orix `Rotation`'s `.data` works as is).  Returns an
        `EBSD` whose `data` is a NumPy array (`compute=True`) or a lazy
        `ProjectedDictionary` (`compute=False`, the default, like the
        reference's `LazyEBSD`), with `xmap` holding the rotations.  `chunk_shape`
        in `kwargs` sets the number of patterns per lazy chunk."""
        self._is_suitable_for_projection(raise_if_not=True)
        rot = np.asarray(getattr(rotations, "data", rotations), dtype=np.float64)
        if detector.navigation_size != 1 and rot.shape[:-1] != detector.navigation_shape:
            raise ValueError(
                "`detector.navigation_shape` must be equal to `rotations.shape`, or the"
                " detector must have exactly one projection center"
            )
        if rot.shape[-1] != 4:
            raise ValueError("`rotations` must be an array of quaternions with a last axis of size 4")
        nav_shape = rot.shape[:-1] if rot.ndim > 1 else (1,)
        if len(nav_shape) > 2:
            raise ValueError(
                "`rotations` can only have one or two dimensions, but an instance with "
                f"{len(nav_shape)} dimensions was passed"
            )
        dtype_out = np.dtype(dtype_out)
        # signals/ebsd_master_pattern.py:224-233
        if dtype_out != self.data.dtype:
            rescale = True
            out_min, out_max = DTYPE_RANGE[dtype_out]
        else:
            rescale = False
            out_min, out_max = 1, 2
        master_upper, master_lower = self._get_master_pattern_arrays_from_energy(energy)
        # one PC per rotation (signals/ebsd_master_pattern.py:236-241, :274-283: `nav_shape_det != (1,)`): the lazy
        # dictionary carries the PCs and every chunk is projected with them on the device, inside the indexing loop
        pcs = detector.pc_flattened if detector.navigation_size != 1 else None
        lazy = ProjectedDictionary(np.ascontiguousarray(master_upper), np.ascontiguousarray(master_lower),
                                   rot.reshape(-1, 4), detector, rescale, out_min, out_max, dtype_out,
                                   device=self._device, chunk=kwargs.get("chunk_shape"), pcs=pcs)
        xmap = DictionaryXmap(rot.reshape(-1, 4), self.phase_name)
        if compute:
            data = lazy.compute().reshape(nav_shape + detector.shape)
        elif len(nav_shape) == 1:
            data = lazy
        else:
            raise NotImplementedError("lazy output needs a 1D array of rotations (pass compute=True)")
        out = EBSD(data, xmap=xmap, device=self._device)
        out.detector = detector
        return out
