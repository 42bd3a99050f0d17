"""PCA ("SVD") decomposition of a stack of patterns on the GPU and the model rebuilt from some of its components - the
numeric steps of the reference's multivariate-analysis workflow (`EBSD.decomposition(algorithm="SVD", ...)`, which is
HyperSpy's, and `EBSD.get_decomposition_model`, signals/ebsd.py:2665-2723, signals/util/_dask.py:283-332).

With X the (patterns x pixels) matrix of M patterns of K pixels and Xc its centred form, the device computes the
float64 Gram matrix of Xc over its SHORTER side and the two skinny products (csrc/decomp.hip); the symmetric
eigen-solve of the side x side matrix runs here, in `numpy.linalg.eigh` - its cost does not grow with the map.

    K <= M:  Xc^T Xc = V L V^T;  factors = V[:, :c],  loadings = Xc factors
    K >  M:  Xc Xc^T = U L U^T;  loadings = U[:, :c] sqrt(L),  factors = Xc^T U[:, :c] / sqrt(L)

`explained_variance` = max(L, 0) / M of all `side` eigenvalues in descending order.  Each factor is flipped so that its
entry of largest magnitude (the first of them on a tie) is positive, its loading with it.  A component whose eigenvalue
is at most side * 2^-52 * L_1 carries rounding noise only: it is null, its factor and loading are exactly zero.

The Gram matrix is formed in float64 because forming it squares the condition number: the components near a typical
cut-off have eigenvalues 1e-4 to 1e-6 of the first, which float32 sums over tens of thousands of patterns would lose
(DESIGN.md §16)."""

import numpy as np

from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import _pattern

CENTRES = {None: _lib.CENTRE_NONE, "navigation": _lib.CENTRE_NAVIGATION, "signal": _lib.CENTRE_SIGNAL}


class LearningResults:
    """What a decomposition leaves behind (the fields of HyperSpy's `LearningResults` that the workflow reads):
    `factors` (K, c) - the component patterns, one per column; `loadings` (M, c); `explained_variance` and
    `explained_variance_ratio` of all min(M, K) components; `mean` - what centring removed (None, the K-vector of the
    mean pattern for "navigation", the M-vector of the patterns' means for "signal"); `centre`; `output_dimension`;
    and the data shape the results belong to."""

    def __init__(self, factors=None, loadings=None, explained_variance=None, explained_variance_ratio=None, mean=None,
                 centre=None, output_dimension=None, data_shape=None):
        self.factors = factors
        self.loadings = loadings
        self.explained_variance = explained_variance
        self.explained_variance_ratio = explained_variance_ratio
        self.mean = mean
        self.centre = centre
        self.output_dimension = output_dimension
        self.data_shape = data_shape
        self.decomposition_algorithm = None if factors is None else "SVD"

    def __repr__(self):
        if self.factors is None:
            return "<LearningResults: empty>"
        return (f"<LearningResults: SVD, {self.factors.shape[1]} components, centre {self.centre!r}, "
                f"factors {self.factors.shape}, loadings {self.loadings.shape}>")


def check_centre(centre):
    if centre is not None and centre not in ("navigation", "signal"):
        raise NotImplementedError(f"centre={centre!r}: None, 'navigation' or 'signal'")
    return CENTRES[centre]


def check_output_dimension(output_dimension, side):
    """`output_dimension` (None: all `side` components) as an int in [1, side]."""
    if output_dimension is None:
        return int(side)
    if isinstance(output_dimension, bool) or not isinstance(output_dimension, (int, np.integer)):
        raise ValueError(f"output_dimension {output_dimension!r} must be a positive integer or None")
    if not 1 <= output_dimension <= side:
        raise ValueError(f"output_dimension {output_dimension} must be between 1 and min(patterns, pixels) = {side}")
    return int(output_dimension)


def check_float_patterns(dtype):
    if np.dtype(dtype).kind != "f":
        raise TypeError(f"To perform a decomposition the data must be of the float type, but the current type is "
                        f"'{np.dtype(dtype)}'. To fix this issue, you can change the type using "
                        "change_dtype('float32') first.")


def null_threshold(eigenvalues_descending, side):
    """Eigenvalues at or below this are rounding noise of the Gram matrix."""
    return side * 2.0 ** -52 * max(float(eigenvalues_descending[0]), 0.0)


def fix_signs(factors, loadings):
    """Flip every factor whose entry of largest magnitude (the first on a tie) is negative, and its loading."""
    if factors.shape[1] == 0:
        return
    rows = np.argmax(np.abs(factors), axis=0)  # (argmax returns the first maximum)
    flip = factors[rows, np.arange(factors.shape[1])] < 0
    factors[:, flip] *= -1.0
    loadings[:, flip] *= -1.0


def results_from_gram(gram, transposed, apply, m, c):
    """factors (K, c), loadings (M, c), explained variance and ratio from the Gram matrix `gram` of the centred patterns
    (`transposed`: Xc Xc^T); `apply(basis, transposed_op)` gives Xc basis or Xc^T basis."""
    side = gram.shape[0]
    lam, vec = np.linalg.eigh(gram)
    lam, vec = lam[::-1], vec[:, ::-1]  # descending
    variance = np.maximum(lam, 0.0) / m
    total = variance.sum()
    ratio = variance / total if total > 0 else np.zeros_like(variance)  # (constant patterns: no variance to share out)
    null = lam[:c] <= null_threshold(lam, side)
    top = np.ascontiguousarray(vec[:, :c])
    if transposed:
        s = np.sqrt(np.where(null, 1.0, lam[:c]))
        loadings = top * s
        factors = apply(top, True) / s
    else:
        factors = top
        loadings = apply(top, False)
    factors[:, null] = 0.0
    loadings[:, null] = 0.0
    fix_signs(factors, loadings)
    return factors, loadings, variance, ratio


def check_decomposition(shape, dtype, output_dimension, centre):
    """What `decomposition_stack` refuses, before any GPU work: (centre code, patterns M, components c)."""
    code = check_centre(centre)
    check_float_patterns(dtype)
    if len(shape) < 2:
        raise ValueError("patterns need at least the two detector axes")
    k = int(shape[-2] * shape[-1])
    m = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
    side = min(m, k)
    c = check_output_dimension(output_dimension, side)
    if side > _lib.DECOMPOSITION_MAX_SIDE:
        raise ValueError(f"decomposition of {m} patterns of {k} pixels needs the eigen-solve of a {side} x {side} matrix on "
                         f"the host, above the limit of {_lib.DECOMPOSITION_MAX_SIDE}: bin the patterns first "
                         "(EBSD.downsample)")
    return code, m, c


def decomposition_stack(patterns, output_dimension=None, centre=None, *, context=None):
    """Decompose the stack `patterns` (..., sy, sx) of float32 / float64 into `output_dimension` principal components
    (None: all min(patterns, pixels)) after the centring `centre` (None, "navigation": subtract the mean pattern,
    "signal": subtract every pattern's own mean): a `LearningResults` of float64 arrays.  Integer patterns are refused as
    HyperSpy refuses them."""
    patterns = np.asarray(patterns)
    checked = check_decomposition(patterns.shape, patterns.dtype, output_dimension, centre)
    return _decompose(patterns, checked, centre, context)


def _decompose(patterns, checked, centre, context):
    """`decomposition_stack` after its checks (`checked`: what `check_decomposition` returned)."""
    code, m, c = checked
    ctx = patterns.context if isinstance(patterns, _pattern.ResidentPatterns) else _pattern._context(context, 0)
    try:
        _pattern._upload(ctx, patterns)
        gram, mean, transposed = ctx.decomposition_gram(code)
        factors, loadings, variance, ratio = results_from_gram(
            gram, transposed, lambda basis, t: ctx.decomposition_apply(basis, code, t), m, c)
    finally:
        if context is None and not isinstance(patterns, _pattern.ResidentPatterns):
            ctx.close()
    return LearningResults(factors, loadings, variance, ratio, mean, centre, c, tuple(patterns.shape))


def select_components(learning_results, components, dtype_out):
    """signals/util/_dask.py:283-332 (`_update_learning_results`): factors and loadings cast to `dtype_out`, then the
    columns `[:, :components]` (None: all, an int: the first ones) or `[:, components]` (a list)."""
    dtype_out = np.dtype(dtype_out)
    factors = learning_results.factors.astype(dtype_out)
    loadings = learning_results.loadings.astype(dtype_out)
    if hasattr(components, "__iter__"):
        factors = factors[:, components]
        loadings = loadings[:, components]
    else:
        factors = factors[:, :components]
        loadings = loadings[:, :components]
    return factors, loadings


def check_model(patterns_shape, learning_results, components, dtype_out):
    """What `decomposition_model_stack` refuses, before any GPU work: (factors, loadings) of the chosen components in
    `dtype_out`."""
    dtype_out = np.dtype(dtype_out)
    if dtype_out not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError(f"dtype_out {dtype_out} is not supported: the decomposition model is float32 or float64")
    lr = learning_results
    if lr is None or lr.factors is None or lr.loadings is None:
        raise ValueError("No learning results found: run a decomposition first")
    shape = tuple(patterns_shape)
    if lr.data_shape is not None and tuple(lr.data_shape) != shape:
        raise ValueError(f"The data of shape {shape} do not match the learning results, which belong to data of shape "
                         f"{tuple(lr.data_shape)}: run the decomposition again")
    factors, loadings = select_components(lr, components, dtype_out)
    if factors.shape[1] < 1:
        raise ValueError(f"components={components!r} selects no component")
    return factors, loadings


def decomposition_model_stack(patterns, learning_results, components=None, dtype_out="float32", *, context=None):
    """The stack rebuilt from the chosen components, loadings factors^T plus the mean that centring removed, summed in
    float64 on the GPU and rounded once to `dtype_out` (float32 / float64), in the shape of `patterns` - the stack the
    results were made from, which the model replaces on the device.  The model needs only the shape of `patterns`, yet
    the stack is uploaded in full (at 40 000 patterns of 60 x 60 a host-to-device copy of 144 MB as uint8, 576 MB as float32, per
    call, of which the model overwrites every value): the device calls work on a resident set, and the upload is what puts the
    context into a known state (problem, dtype, no recorded background step left over)."""
    patterns = np.asarray(patterns)
    checked = check_model(patterns.shape, learning_results, components, dtype_out)
    return _model(patterns, checked, learning_results, dtype_out, context)


def _model(patterns, checked, learning_results, dtype_out, context):
    """`decomposition_model_stack` after its checks (`checked`: what `check_model` returned)."""
    factors, loadings = checked
    ctx = patterns.context if isinstance(patterns, _pattern.ResidentPatterns) else _pattern._context(context, 0)
    try:
        _pattern._upload(ctx, patterns)
        ctx.decomposition_model(loadings, factors, learning_results.mean, CENTRES[learning_results.centre], dtype_out)
        if isinstance(patterns, _pattern.ResidentPatterns):
            return patterns.result()
        return ctx.get_experimental().reshape(patterns.shape)
    finally:
        if context is None and not isinstance(patterns, _pattern.ResidentPatterns):
            ctx.close()
