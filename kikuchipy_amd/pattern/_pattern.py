"""Static / dynamic background removal, FFT filtering, intensity rescaling / normalization and image quality on the GPU.

Array-level counterparts of `EBSD.remove_static_background`
(signals/ebsd.py:442-573) and `EBSD.remove_dynamic_background`
(signals/ebsd.py:575-696): same arguments, defaults, validation messages and
output dtype; the per-pattern kernels of pattern/_pattern.py:392-509 run as
one HIP workgroup per pattern (csrc/preproc.hip).  `get_image_quality`
(pattern/_pattern.py:698-775) runs a half-spectrum DFT per pattern
(csrc/iq.hip).  `fft_filter_stack` is what `EBSD.fft_filter`
(signals/ebsd.py:805-930) runs on a stack (csrc/fftfilter.hip).
`rescale_intensity` / `normalize_intensity` (pattern/_pattern.py:31-93,
:154-210) and their `_stack` forms, which `EBSD.rescale_intensity` /
`normalize_intensity` (signals/_kikuchipy_signal.py:88-338) run, map every
pattern in one HIP workgroup (csrc/intensity.hip).  `adaptive_histogram_equalization` (pattern/_pattern.py:810-840)
and `adaptive_histogram_equalization_stack`, which `EBSD.adaptive_histogram_equalization`
(signals/_kikuchipy_signal.py:340-470) runs, equalize every pattern in one HIP workgroup (csrc/clahe.hip).
`downsample_stack` (signals/ebsd.py:1113-1219) bins every pattern and changes the detector shape
(csrc/downsample.hip); `get_dynamic_background` / `get_dynamic_background_stack` (pattern/_pattern.py:634-695,
signals/ebsd.py:698-803) return the blur that `remove_dynamic_background` removes (csrc/preproc.hip).
"""

import numbers
import operator

import numpy as np

from kikuchipy_amd import _lib

_OPS = {"subtract": _lib.OP_SUBTRACT, "divide": _lib.OP_DIVIDE}
_DOMAINS = {"frequency": _lib.DOMAIN_FREQUENCY, "spatial": _lib.DOMAIN_SPATIAL}
_SUPPORTED = (np.uint8, np.uint16, np.int8, np.int16, np.float32, np.float64)


def _context(context, device):
    return context if context is not None else _lib.Context(device)


class ResidentPatterns:
    """The patterns of a resident `EBSD` signal (`EBSD.to_device`): they live in the HBM of `context` as its experimental
    set, which nothing else may upload into.  Stands in for the host array in every stack function of this package:
    `shape`, `dtype` and `ndim` follow the context (an op may change the detector shape or the dtype), `_upload` finds
    the patterns in place, and with `keep` a function that would download the processed patterns returns this object
    instead - they stay where they are."""

    def __init__(self, context, navigation_shape, keep=False):
        self.context = context
        self.navigation_shape = tuple(int(n) for n in navigation_shape)
        self.keep = keep

    def kept(self, keep=True):
        return ResidentPatterns(self.context, self.navigation_shape, keep)

    def flat(self):
        """As a stack (n, sy, sx)."""
        return ResidentPatterns(self.context, (int(self.context._exp_shape[0]),), self.keep)

    shape = property(lambda self: self.navigation_shape + tuple(self.context._detector))
    dtype = property(lambda self: np.dtype(self.context._exp_dtype))
    ndim = property(lambda self: len(self.navigation_shape) + 2)
    size = property(lambda self: int(np.prod(self.shape)))

    def host(self):
        """A host copy (the recorded background steps run first)."""
        return self.context.get_experimental().reshape(self.shape)

    def result(self, collect=None):
        """What a stack function returns after its op ran on the context: this object (`keep`), else what `collect`
        (default: a download of the patterns) gives, one row per pattern, in the navigation shape."""
        if collect is None:
            if self.keep:
                return self
            collect = _download
        out = collect(self.context)
        return out.reshape(self.navigation_shape + out.shape[1:])


def as_patterns(patterns):
    """`np.asarray`, except that resident patterns pass through."""
    return patterns if isinstance(patterns, ResidentPatterns) else np.asarray(patterns)


def _upload(ctx, patterns):
    if isinstance(patterns, ResidentPatterns):
        if ctx is not patterns.context:
            raise ValueError("resident patterns are processed on the context that holds them")
        if patterns.dtype.type not in _SUPPORTED:
            raise ValueError(f"pattern dtype {patterns.dtype} is not supported by the GPU pre-processing kernels")
        sy, sx = patterns.shape[-2:]
        ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)  # (keeps the patterns; a signal mask of an indexing run goes)
        return patterns.shape
    patterns = np.asarray(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    if patterns.dtype.type not in _SUPPORTED:
        raise ValueError(f"pattern dtype {patterns.dtype} is not supported by the GPU pre-processing kernels")
    sy, sx = patterns.shape[-2:]
    flat = np.ascontiguousarray(patterns).reshape((-1, sy, sx))
    ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
    ctx.set_experimental(flat)
    return patterns.shape


def _download(ctx):
    return ctx.get_experimental()


def _process(patterns, record, context, device, contexts, collect=_download):
    """Upload -> `record(ctx)` (the recorded step) -> `collect(ctx)` (one row per pattern), on one context or -
    `contexts`: one per GPU, the members of a `_lib.Group` - block-wise: the patterns are independent, every GPU takes a
    contiguous block of them over its own host link from a host thread of its own (the library calls release the GIL);
    the blocks are concatenated and given the patterns' leading shape.  `ResidentPatterns` are processed where they are,
    without the upload - and without the download when they are to be kept."""
    if isinstance(patterns, ResidentPatterns):
        _upload(patterns.context if context is None else context, patterns)
        record(patterns.context)
        return patterns.result(None if collect is _download else collect)
    patterns = np.asarray(patterns)
    lead = patterns.shape[:-2]
    if contexts and len(contexts) > 1 and patterns.ndim > 2 and int(np.prod(patterns.shape[:-2])) >= len(contexts):
        from concurrent.futures import ThreadPoolExecutor

        from kikuchipy_amd.parallel import shard_range

        flat = np.ascontiguousarray(patterns).reshape((-1,) + patterns.shape[-2:])
        blocks = [shard_range(len(flat), i, len(contexts)) for i in range(len(contexts))]

        def one(job):
            c, (a, b) = job
            _upload(c, flat[a:b])
            record(c)
            return collect(c)

        with ThreadPoolExecutor(len(contexts)) as pool:
            parts = list(pool.map(one, zip(contexts, blocks)))
        return np.concatenate(parts, axis=0).reshape(lead + parts[0].shape[1:])
    ctx = contexts[0] if contexts else _context(context, device)
    try:
        _upload(ctx, patterns)
        record(ctx)
        out = collect(ctx)
        return out.reshape(lead + out.shape[1:])
    finally:
        if context is None and not contexts:
            ctx.close()


def check_static_background(patterns_dtype, sig_shape, static_bg):
    """Validation of signals/ebsd.py:525-546."""
    if not isinstance(static_bg, np.ndarray):
        if hasattr(static_bg, "compute"):
            static_bg = static_bg.compute()
        else:
            raise ValueError("`EBSD.static_background` is not a valid array")
    dtype_out = np.dtype(patterns_dtype).type
    if dtype_out != static_bg.dtype:
        raise ValueError(
            f"Static background dtype_out {static_bg.dtype} is not the same as "
            f"pattern dtype_out {dtype_out}"
        )
    if static_bg.shape != tuple(sig_shape):
        raise ValueError(
            f"Signal {tuple(sig_shape)} and static background {static_bg.shape} shapes are not "
            "the same"
        )
    return static_bg.astype(np.float32)


def remove_static_background(patterns, static_bg, operation="subtract", scale_bg=False, *,
                             context=None, device=0, contexts=None):
    """Remove the static background from every pattern; returns a new array of
    the input dtype.  `static_bg` must have the patterns' dtype and detector
    shape, as in the reference."""
    if operation not in _OPS:
        raise ValueError(f"operation '{operation}' must be either 'subtract' or 'divide'")
    patterns = as_patterns(patterns)
    bg = check_static_background(patterns.dtype, patterns.shape[-2:], static_bg)
    return _process(patterns, lambda c: c.remove_static_background(bg, _OPS[operation], scale_bg), context, device, contexts)


def remove_dynamic_background(patterns, operation="subtract", filter_domain="frequency", std=None,
                              truncate=4.0, *, context=None, device=0, contexts=None):
    """Remove the dynamic background (Gaussian blur of each pattern, by
    subtraction or division) from every pattern; returns a new array of the
    input dtype.  `std` defaults to an eighth of the pattern width."""
    if filter_domain not in _DOMAINS:
        raise ValueError(f"{filter_domain} must be either of {list(_DOMAINS)}")
    if operation not in _OPS:
        raise ValueError(f"operation '{operation}' must be either 'subtract' or 'divide'")
    patterns = as_patterns(patterns)
    if std is None:
        std = patterns.shape[-1] / 8
    return _process(patterns, lambda c: c.remove_dynamic_background(_OPS[operation], _DOMAINS[filter_domain], std, truncate),
                    context, device, contexts)


def fft_frequency_vectors(shape):
    """The weight of every frequency of a 2-D DFT spectrum of `shape` (pattern/_pattern.py:365-386): float64
    `ly[k]**2 + lx[l]**2 - 1` with `lx = arange(sx) + 1`, `lx[sx // 2:] -= sx + 1` (`ly` alike).  Not symmetric under
    (k, l) -> (-k, -l); that is the reference's convention."""
    sy, sx = shape
    linex = np.arange(sx) + 1
    linex[sx // 2:] -= sx + 1
    liney = np.arange(sy) + 1
    liney[sy // 2:] -= sy + 1
    return (liney[:, None] ** 2 + linex[None, :] ** 2 - 1).astype(np.float64)


def get_image_quality(patterns, normalize=True, frequency_vectors=None, inertia_max=None, *,
                      context=None, device=0, contexts=None):
    """Image quality Q of Krieger Lassen (pattern/_pattern.py:698-775) of one pattern (a Python float) or of every
    pattern of a stack (..., sy, sx) (float32 of the leading shape):
    `Q = 1 - (sum |F| w / sum |F|) / inertia_max`, F the 2-D DFT of the pattern as float32, after subtracting its mean
    when `normalize`.  `frequency_vectors` (sy, sx) default to `fft_frequency_vectors`, `inertia_max` to
    `sum(frequency_vectors) / (sy * sx)`.

    NaN where the reference's arithmetic gives 0/0 or meets a non-finite value: a pattern holding a NaN or inf, an
    all-zero pattern without `normalize`, and, with `normalize`, a pattern whose values are all exactly equal.  For
    float patterns of equal values whose float32 mean is not exact the reference divides round-off by round-off and
    returns noise instead; here such a pattern is NaN too."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    sig = patterns.shape[-2:]
    w = None
    if frequency_vectors is not None:
        w = np.asarray(frequency_vectors, dtype=np.float64)
        if w.shape != sig:
            raise ValueError(f"frequency_vectors have shape {w.shape}, the patterns {sig}")
    if inertia_max is None:
        inertia_max = 0.0  # derived from the weights by the library
    elif not inertia_max > 0:
        raise ValueError(f"inertia_max must be positive, not {inertia_max}")
    q = _process(patterns, lambda c: None, context, device, contexts,
                 collect=lambda c: c.image_quality(normalize, w, inertia_max))
    return float(q) if patterns.ndim == 2 else q


def region_sums(patterns, rects, *, context=None, device=0, contexts=None):
    """`np.nansum(patterns[..., row0:row1, col0:col1], axis=(-2, -1))` for every rectangle (row0, row1, col0, col1) of
    `rects` (n_rects, 4) - half-open, inside the detector, free to overlap or be empty - in one pass over the patterns
    (csrc/regionsum.hip): an array of shape `patterns.shape[:-2] + (n_rects,)`, uint64 for uint8 / uint16 patterns,
    int64 for int8 / int16 (both exact), float32 / float64 for patterns of these (summed in float64 in a fixed order
    and rounded once; NaN counts as 0).  The same bits whichever way `contexts` split the patterns."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    r = np.asarray(rects)
    if r.size == 0:
        r = r.reshape(0, 4)
    if r.ndim != 2 or r.shape[1] != 4 or r.dtype.kind not in "iu":
        raise ValueError(f"rects must be integers of shape (n_rects, 4): (row0, row1, col0, col1), not {r.dtype} {r.shape}")
    sy, sx = patterns.shape[-2:]
    bad = (r[:, 0] < 0) | (r[:, 1] < r[:, 0]) | (r[:, 1] > sy) | (r[:, 2] < 0) | (r[:, 3] < r[:, 2]) | (r[:, 3] > sx)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"rectangle {k}, {tuple(int(v) for v in r[k])}, is not inside the {sy} x {sx} detector")
    r = np.ascontiguousarray(r, dtype=np.int32)
    return _process(patterns, lambda c: None, context, device, contexts, collect=lambda c: c.region_sums(r))


def reduce_stack(patterns, op, axes, *, context=None, device=0, contexts=None):
    """`getattr(np, op)(patterns, axis=axes)` for `op` "sum", "mean", "max", "min", "std" or "var" over the array axes
    `axes` (ints, negative ones from the end, each once) of patterns with up to two leading axes, on the GPU
    (csrc/reduce.hip): NumPy's result shape and dtype (`_lib.reduce_dtype`).  Integer sums, means, maxima and minima
    are NumPy's bits; integer std / var come from the exact sums of x and x^2; float patterns are accumulated in
    float64 in a fixed order and rounded once, NaN propagates.  A reduction over detector axes only splits over
    `contexts` like the other read-only ops, with the same bits; one that takes in a leading axis runs on one context
    (partial sums of several GPUs would be combined in another order) and refuses more."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2 or patterns.ndim > 4:
        raise ValueError("patterns need the two detector axes and at most two leading axes")
    _lib.reduce_dtype(patterns.dtype, op)  # (refuses an unknown op)
    if isinstance(axes, numbers.Integral):
        axes = (axes,)
    reduced = set()
    for ax in axes:
        if not isinstance(ax, numbers.Integral) or isinstance(ax, bool) or not -patterns.ndim <= ax < patterns.ndim:
            raise ValueError(f"axis {ax!r} is out of bounds for patterns of {patterns.ndim} axes")
        reduced.add(int(ax) % patterns.ndim)
    if not reduced:
        raise ValueError("no axis to reduce over")
    lead = patterns.ndim - 2
    if min(reduced) >= lead:  # every pattern on its own: a stack (n, sy, sx) per context
        per_pattern = [ax - lead + 1 for ax in sorted(reduced)]
        return _process(patterns, lambda c: None, context, device, contexts,
                        collect=lambda c: c.reduce(op, per_pattern, (c._exp_shape[0],)))
    if contexts and len(contexts) > 1:
        raise ValueError("a reduction over a navigation axis runs on one GPU")
    if isinstance(patterns, ResidentPatterns):
        _upload(patterns.context if context is None else context, patterns)
        return patterns.context.reduce(op, sorted(reduced), patterns.navigation_shape)
    ctx = contexts[0] if contexts else _context(context, device)
    try:
        _upload(ctx, patterns)
        return ctx.reduce(op, sorted(reduced), patterns.shape[:-2])
    finally:
        if context is None and not contexts:
            ctx.close()


_FUNCTION_DOMAINS = ["frequency", "spatial"]


def fft_filter_table(transfer_function, function_domain, shift, shape):
    """(domain code, table) of `Context.fft_filter` for patterns of `shape` (sy, sx), with the reference's checks.

    Frequency domain: the reference computes `Re(ifft2(fft2(p) H'))` with `H' = ifftshift(H)` for `shift` (its
    fftshift -> multiply -> ifftshift, for odd shapes too), else `H`.  For real `p` that equals `ifft2(fft2(p) Hs)` with
    `Hs(k) = (H'(k) + conj(H'(-k))) / 2`, so `H` may be complex or not symmetric; the table is `Hs` on the half
    spectrum, (sy, sx // 2 + 1) complex.  Spatial domain: the kernel (ty, tx) as float64."""
    if function_domain == "frequency":
        h = np.asarray(transfer_function)
        if h.shape != tuple(shape):
            raise ValueError(f"transfer_function has shape {h.shape}, the patterns {tuple(shape)}")
        h = np.asarray(np.fft.ifftshift(h) if shift else h, dtype=np.complex128)
        sy, sx = h.shape
        mirror = np.conj(h[(-np.arange(sy)) % sy][:, (-np.arange(sx)) % sx])
        return _lib.DOMAIN_FREQUENCY, (0.5 * (h + mirror))[:, : sx // 2 + 1]
    if function_domain == "spatial":
        w = np.asarray(transfer_function)
        if w.ndim != 2 or np.iscomplexobj(w):
            raise ValueError(f"a spatial kernel must be a real 2D array, not of shape {w.shape} and dtype {w.dtype}")
        return _lib.DOMAIN_SPATIAL, w.astype(np.float64)
    raise ValueError(f"{function_domain} must be either of {_FUNCTION_DOMAINS}")


def fft_filter_stack(patterns, transfer_function, function_domain, shift=False, *, context=None, device=0,
                     contexts=None):
    """`EBSD.fft_filter` on an array (..., sy, sx): every pattern as float32, filtered
    (`fft_filter_table`), then `rescale_intensity(filtered, dtype_out=patterns.dtype)`; returns a new array of the
    input's dtype and shape.  A pattern holding a NaN or inf, or whose filtered result is constant (the reference's
    0 / 0), becomes 0 for integer dtypes and NaN for float dtypes.

    Not the reference's `pattern.fft_filter`, which returns one unrescaled float pattern."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    domain, table = fft_filter_table(transfer_function, function_domain, shift, patterns.shape[-2:])
    return _process(patterns, lambda c: c.fft_filter(domain, table), context, device, contexts)


# skimage.util.dtype.dtype_range (skimage need not be importable): the default out_range of rescale_intensity
DTYPE_RANGE = {
    np.bool_: (False, True),
    np.float16: (-1, 1),
    np.float32: (-1, 1),
    np.float64: (-1, 1),
    np.uint8: (0, 255),
    np.uint16: (0, 65535),
    np.uint32: (0, 2**32 - 1),
    np.uint64: (0, 2**64 - 1),
    np.int8: (-128, 127),
    np.int16: (-32768, 32767),
    np.int32: (-(2**31), 2**31 - 1),
    np.int64: (-(2**63), 2**63 - 1),
}
INTENSITY_DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.float32, np.float64)


def intensity_dtype_out(dtype_out, default):
    """`dtype_out` (None: `default`) as a NumPy dtype the intensity kernels write, else ValueError."""
    dt = np.dtype(default) if dtype_out is None else np.dtype(dtype_out)
    if dt.type not in INTENSITY_DTYPES:
        raise ValueError(f"dtype_out {dt} is not supported: the GPU intensity kernels write "
                         f"{', '.join(np.dtype(t).name for t in INTENSITY_DTYPES)}")
    return dt


def _out_range(out_range, dtype_out):
    return DTYPE_RANGE[dtype_out.type] if out_range is None else tuple(out_range)


def _check_percentiles(percentiles):
    q = np.asarray(percentiles, dtype=np.float64)
    if q.shape != (2,):
        raise ValueError(f"percentiles must be a pair, not {percentiles!r}")
    if not np.all((q >= 0) & (q <= 100)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    return q


def _rescale_record(in_range, out_range, dtype_out, percentiles):
    omin, omax = out_range
    return lambda c, rng=in_range: c.rescale_intensity(None if percentiles is not None else rng, percentiles,
                                                       omin, omax, dtype_out)


def _process_relative(patterns, rescale, context, device, contexts):
    """`rescale(ctx, in_range)` with in_range the global (min, max) of all patterns, NaN-propagating as
    `data.min()` / `data.max()`.  One context: upload, reduce, rescale, download.  Several (`contexts`, block-wise as
    `_process`): every member uploads its block and reduces it, the host combines the ranges, then every member
    rescales and downloads its block."""
    patterns = as_patterns(patterns)
    lead = patterns.shape[:-2]
    if not (contexts and len(contexts) > 1 and patterns.ndim > 2 and int(np.prod(lead)) >= len(contexts)):
        return _process(patterns, lambda c: rescale(c, c.intensity_range()), context, device, contexts)
    from concurrent.futures import ThreadPoolExecutor

    from kikuchipy_amd.parallel import shard_range

    flat = np.ascontiguousarray(patterns).reshape((-1,) + patterns.shape[-2:])
    blocks = [shard_range(len(flat), i, len(contexts)) for i in range(len(contexts))]

    def reduce(job):
        c, (a, b) = job
        _upload(c, flat[a:b])
        return c.intensity_range()

    def finish(c):
        rescale(c, rng)
        return _download(c)

    with ThreadPoolExecutor(len(contexts)) as pool:
        ranges = np.array(list(pool.map(reduce, zip(contexts, blocks))))
        rng = np.array([ranges[:, 0].min(), ranges[:, 1].max()])  # NaN in any block -> NaN
        parts = list(pool.map(finish, contexts))
    return np.concatenate(parts, axis=0).reshape(lead + parts[0].shape[1:])


def rescale_intensity(pattern, in_range=None, out_range=None, dtype_out=None, percentiles=None, *, context=None,
                      device=0):
    """pattern/_pattern.py:31-93: `((clip(p, imin, imax) - imin) / (imax - imin)) * (omax - omin) + omin` as
    `dtype_out` (default: the pattern's dtype), with (imin, imax) = `np.nanpercentile(p, percentiles)` (which overwrites
    `in_range`), else `in_range`, else the pattern's nanmin / nanmax; (omin, omax) = `out_range`, default the dtype
    range of `dtype_out` (`DTYPE_RANGE`).  As in the reference the whole input is ONE image, whatever its shape.
    NumPy 1.26 arithmetic: float64 for integer and float64 patterns, float32 for float32 patterns; integer patterns
    are computed exactly (the reference's int8 / int16 differences can wrap); casts to integer dtypes truncate to int32
    and keep the low bits (NaN -> 0)."""
    pattern = np.asarray(pattern)
    dt = intensity_dtype_out(dtype_out, pattern.dtype)
    if percentiles is not None:
        percentiles = _check_percentiles(percentiles)
    one = pattern.reshape((1, 1, pattern.size))
    out = _process(one, _rescale_record(in_range, _out_range(out_range, dt), dt, percentiles), context, device, None)
    return out.reshape(pattern.shape)


def normalize_intensity(pattern, num_std=1, divide_by_square_root=False, dtype_out=None, *, context=None, device=0):
    """pattern/_pattern.py:154-210: `(p - mean) / (num_std * std [* sqrt(p.size)])` of the whole input as one image,
    as `dtype_out`; None gives the arithmetic's dtype, float64 (integer and float64 input) or float32 (float32 input).
    Sums run in float64."""
    pattern = np.asarray(pattern)
    arith = np.float32 if pattern.dtype == np.float32 else np.float64
    dt = intensity_dtype_out(dtype_out, arith)
    one = pattern.reshape((1, 1, pattern.size))
    out = _process(one, lambda c: c.normalize_intensity(num_std, divide_by_square_root, dt), context, device, None)
    return out.reshape(pattern.shape)


def rescale_intensity_stack(patterns, in_range=None, out_range=None, dtype_out=None, percentiles=None, *,
                            relative=False, context=None, device=0, contexts=None):
    """`rescale_intensity` of every pattern of (..., sy, sx), what `EBSD.rescale_intensity` maps: `relative` takes
    (imin, imax) as the global min / max of all patterns (NaN if any is NaN) unless `percentiles` are given; returns a
    new array of `dtype_out` (default: the patterns' dtype) and the input's shape."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    dt = intensity_dtype_out(dtype_out, patterns.dtype)
    if percentiles is not None:
        percentiles = _check_percentiles(percentiles)
    record = _rescale_record(in_range, _out_range(out_range, dt), dt, percentiles)
    if relative and percentiles is None:
        return _process_relative(patterns, lambda c, rng: record(c, rng), context, device, contexts)
    return _process(patterns, record, context, device, contexts)


def normalize_intensity_stack(patterns, num_std=1, divide_by_square_root=False, dtype_out=None, *, context=None,
                              device=0, contexts=None):
    """`normalize_intensity` of every pattern of (..., sy, sx), what `EBSD.normalize_intensity` maps; `dtype_out`
    defaults to the patterns' dtype, as there."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    dt = intensity_dtype_out(dtype_out, patterns.dtype)
    return _process(patterns, lambda c: c.normalize_intensity(num_std, divide_by_square_root, dt), context, device,
                    contexts)


def check_binning_factor(factor, sig_shape):
    """The checks of `EBSD.downsample` (signals/ebsd.py:1167-1179) for patterns of `sig_shape` (sy, sx), with its
    messages: shape and remainder in HyperSpy's (x, y) order."""
    if not isinstance(factor, int) or factor <= 1:
        raise ValueError(f"Binning factor {factor} must be an integer > 1")
    sig_shape_old = tuple(int(v) for v in sig_shape[::-1])
    rest = np.mod(sig_shape_old, factor)
    if not all(rest == 0):
        raise ValueError(
            f"Binning factor {factor} must be a divisor of the initial pattern "
            f"shape {sig_shape_old}, but {tuple(int(r) for r in rest)} pixels remain.\n"
            "You might try to crop away these pixels first using EBSD.crop()."
        )
    return int(factor)


def downsample_stack(patterns, factor, dtype_out=None, *, context=None, device=0, contexts=None):
    """`EBSD.downsample` on an array (..., sy, sx): every pattern binned by the integer `factor`, which must divide sy
    and sx, and rescaled to the range of `dtype_out` (default: the patterns' dtype; `DTYPE_RANGE`): a new array
    (..., sy / factor, sx / factor) of `dtype_out`.  The reference's `_downsample2d` (pattern/_pattern.py:776-807) bit
    for bit: float32 sums in its order, float32 rescaling, `astype`.  A pattern holding a NaN, or whose binned image is
    constant (the reference's 0 / 0), becomes NaN for float `dtype_out` and 0 for integer ones (csrc/downsample.hip)."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    factor = check_binning_factor(factor, patterns.shape[-2:])
    dt = intensity_dtype_out(dtype_out, patterns.dtype)
    return _process(patterns, lambda c: c.downsample(factor, dt), context, device, contexts)


def get_dynamic_background_stack(patterns, filter_domain="frequency", std=None, truncate=4.0, dtype_out=None, *,
                                 context=None, device=0, contexts=None):
    """`EBSD.get_dynamic_background` on an array (..., sy, sx): the Gaussian-blurred image of every pattern - what
    `remove_dynamic_background` subtracts or divides away - as `dtype_out` (default: the patterns' dtype).  As in the
    reference (signals/ebsd.py:767-779) the patterns are cast to `dtype_out` first.  "frequency": the cast pattern as
    float32 through the FFT filter's correlation with a Gaussian window of int(truncate * std) samples, stored into
    `dtype_out` (integers truncate); within the FFT's float32 round-off of the reference.  "spatial":
    `scipy.ndimage.gaussian_filter(sigma=std, truncate=truncate)` on the cast pattern, whose two passes are each stored
    in `dtype_out`.  `std` defaults to an eighth of the pattern width."""
    if filter_domain not in _DOMAINS:
        raise ValueError(f"{filter_domain} must be either of {list(_DOMAINS)}")
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    dt = intensity_dtype_out(dtype_out, patterns.dtype)
    if std is None:
        std = patterns.shape[-1] / 8
    return _process(patterns, lambda c: None, context, device, contexts,
                    collect=lambda c: c.get_dynamic_background(_DOMAINS[filter_domain], std, truncate, dt))


def get_dynamic_background(pattern, filter_domain="frequency", std=None, truncate=4.0, *, context=None, device=0):
    """pattern/_pattern.py:634-695 on one 2-D pattern: its dynamic background in the pattern's data type; `std`
    defaults to `pattern.shape[1] / 8`."""
    pattern = np.asarray(pattern)
    if pattern.ndim != 2:
        raise ValueError(f"one 2-D pattern is filtered, not an array of shape {pattern.shape}")
    return get_dynamic_background_stack(pattern, filter_domain, std, truncate, context=context, device=device)


CLAHE_MAX_NBINS = 16384  # csrc/clahe_plan.h: 2**14 grey levels


def clahe_kernel_size(kernel_size, sig_shape):
    """The kernel (rows, cols) `EBSD.adaptive_histogram_equalization` derives for patterns of `sig_shape` (sy, sx):
    None gives (sx // 4, sy // 4) - the reference takes HyperSpy's signal_shape (x, y) as (rows, cols), so the default
    is transposed for non-square patterns - a number (k, k), a pair is taken as it is; int() of each entry."""
    sy, sx = sig_shape
    if kernel_size is None:
        kernel_size = (sx // 4, sy // 4)
    elif isinstance(kernel_size, numbers.Number):
        kernel_size = (kernel_size,) * 2
    elif len(kernel_size) != 2:
        raise ValueError(f"Incorrect value of `shape`: {kernel_size}")
    return [int(k) for k in kernel_size]


def clahe_arguments(patterns, kernel_size, clip_limit, nbins):
    """(ky, kx, clip_count, nbins) of `Context.adaptive_histogram_equalization` for `patterns` (..., sy, sx) and a
    kernel of (rows, cols), raising what the reference raises for its first pattern, in its order, before any GPU work:
    a float pattern outside [-1, 1] without a NaN (img_as_uint), a kernel entry of 0 (ZeroDivisionError) or below,
    nbins of 0 (ZeroDivisionError) or below.  nbins above 16384 is refused; the reference accepts it and lets the extra,
    always empty bins take part in the clip redistribution."""
    ky, kx = kernel_size
    if patterns.dtype.kind == "f" and patterns.size:
        if isinstance(patterns, ResidentPatterns):
            patterns = patterns.host()  # (the per-pattern extrema decide: one download)
        flat = patterns.reshape(-1, patterns.shape[-2] * patterns.shape[-1])
        mn, mx = flat.min(axis=1), flat.max(axis=1)  # NaN in a pattern: no check for it, as np.min gives NaN there
        if np.any((mn < -1.0) | (mx > 1.0)):
            raise ValueError("Images of type float must be between -1 and 1.")
    if ky == 0 or kx == 0:
        raise ZeroDivisionError("integer division or modulo by zero")
    if ky < 0 or kx < 0:
        raise ValueError("index can't contain negative values")
    nbins = operator.index(nbins)
    if nbins == 0:
        raise ZeroDivisionError("integer division or modulo by zero")
    if nbins < 0:
        raise ValueError("'minlength' must not be negative")
    if nbins > CLAHE_MAX_NBINS:
        raise ValueError(f"nbins={nbins}: at most {CLAHE_MAX_NBINS} bins (the 2**14 grey levels of the equalization) "
                         "are supported")
    kk = ky * kx
    clim = int(np.clip(clip_limit * kk, 1, None)) if clip_limit > 0 else kk
    return ky, kx, min(clim, kk), nbins  # a limit of ky * kx or more clips nothing


def adaptive_histogram_equalization(pattern, kernel_size, clip_limit=0, nbins=128, *, context=None, device=0):
    """pattern/_pattern.py:810-840 on one 2-D pattern: scikit-image 0.18.3's
    `equalize_adapthist(pattern, kernel_size, clip_limit, nbins)`, then `rescale_intensity` to the range of the pattern's
    dtype; returns a new array of that dtype.  `kernel_size`: None gives scikit-image's default (sy // 8, sx // 8), a
    number (k, k), a pair (rows, cols); a length other than 2 raises (scikit-image builds that error without raising
    it).  Errors: `clahe_arguments`."""
    pattern = np.asarray(pattern)
    if pattern.ndim != 2:
        raise ValueError(f"one 2-D pattern is equalized, not an array of shape {pattern.shape}")
    if kernel_size is None:
        kernel_size = (pattern.shape[0] // 8, pattern.shape[1] // 8)
    elif isinstance(kernel_size, numbers.Number):
        kernel_size = (kernel_size,) * 2
    elif len(kernel_size) != 2:
        raise ValueError(f"Incorrect value of `kernel_size`: {kernel_size}")
    args = clahe_arguments(pattern, [int(k) for k in kernel_size], clip_limit, nbins)
    return _process(pattern, lambda c: c.adaptive_histogram_equalization(*args), context, device, None)


def adaptive_histogram_equalization_stack(patterns, kernel_size=None, clip_limit=0, nbins=128, *, context=None,
                                          device=0, contexts=None):
    """`adaptive_histogram_equalization` of every pattern of (..., sy, sx), what
    `EBSD.adaptive_histogram_equalization` maps: `kernel_size` as `clahe_kernel_size` derives it (None: the reference's
    (sx // 4, sy // 4)); returns a new array of the input's dtype and shape."""
    patterns = as_patterns(patterns)
    if patterns.ndim < 2:
        raise ValueError("patterns need at least the two detector axes")
    args = clahe_arguments(patterns, clahe_kernel_size(kernel_size, patterns.shape[-2:]), clip_limit, nbins)
    return _process(patterns, lambda c: c.adaptive_histogram_equalization(*args), context, device, contexts)
