"""The cases of the bit-for-bit tests of the FFT filter and image quality (tests/test_host_spectral.py,
tests/test_gpu_spectral_kernels.py): named (operation, shape, dtype, transfer function or kernel, n, path, batch cap)
with deterministic inputs from tests/_iq_inputs.py's integer hash and the builders of tests/_fft_filter_cases.py, and the
restatement (tests/_spectral_restate.py) of each, computed once and shared.

`path` is the kernel path a case claims to run on; `forced` says that it gets there by KPDI_FFT_FILTER_PATH=1 /
KPDI_IQ_PATH=1, `batch` that KPDI_PATTERN_BATCH caps a workspace batch.  test_host_spectral.py holds these claims to
csrc/fftfilter_plan.h and csrc/iq_plan.h compiled on the host."""

import functools
import os
from collections import namedtuple

import numpy as np

import _fft_filter_cases as ff_cases
import _iq_inputs
import _spectral_restate as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = ["uint8", "int8", "uint16", "int16", "float32", "float64"]
OPS = ["frequency", "spatial", "iq"]
SWITCHES = ("KPDI_FFT_FILTER_PATH", "KPDI_IQ_PATH", "KPDI_PATTERN_BATCH")
LDS_CAP = 150 * 1024  # PATTERN_LDS_CAP of csrc/pattern_plan.h

Case = namedtuple("Case", "name op shape dtype n tf path forced batch normalize weights kind seed")

SMALL = [(2, 2), (3, 5), (4, 6), (5, 8), (8, 5), (1, 64), (64, 1), (7, 9), (6, 7), (5, 5), (60, 60), (61, 59)]
WIDE = [(17, 300), (300, 3)]  # an axis longer than the 256 threads, several workgroups per pattern on path 1
FREQ_TF = ["lowhigh", "complex", "nonsym"]
SPATIAL_TF = ["sobel", "even4", "big", "one"]
# the first shape path 0 does not take, square; the one before it is the last it takes (asserted by the host test
# against the compiled plan headers)
BOUNDARY = {"frequency": 112, "spatial": 139, "iq": 138}


# ---- what the plan headers say, restated for the bookkeeping ----------------------------------------------------------
def lds_path_bytes(op, sy, sx):
    npix, inter = sy * sx, sy * (sx // 2 + 1)
    pix4 = (npix + 3) // 4 * 4
    if op == "spatial":
        return 2 * pix4 * 4 + 128
    if op == "frequency":
        return pix4 * 4 + 2 * inter * 8 + (sx + sy) * 8 + 128
    return (npix + 1) // 2 * 2 * 4 + inter * 8 + (sx + sy) * 8 + 128


def natural_path(op, shape):
    return 0 if lds_path_bytes(op, *shape) <= LDS_CAP else 1


def batches(c):
    """Number of launches batches of a case: 1 on path 0, else ceil(n / cap)."""
    return 1 if c.path == 0 or not c.batch else -(-c.n // c.batch)


def env(c):
    """The switches of a case."""
    e = {}
    if c.forced:
        e["KPDI_IQ_PATH" if c.op == "iq" else "KPDI_FFT_FILTER_PATH"] = "1"
    if c.batch:
        e["KPDI_PATTERN_BATCH"] = str(c.batch)
    return e


# ---- the table --------------------------------------------------------------------------------------------------------
def _make(cases, tag, op, shape, dtype, tf, path, n=2, batch=None, normalize=True, weights=False, kind="hash", seed=0):
    nat = natural_path(op, shape)
    forced = path == 1 and nat == 0
    assert path == nat or forced, (tag, op, shape, path)
    tf = None if op == "iq" else tf
    name = "-".join(str(v) for v in (tag, op, f"{shape[0]}x{shape[1]}", dtype, tf or ("norm" if normalize else "raw"),
                                     f"p{path}" + (f"b{batch}" if batch else ""), f"n{n}"))
    c = Case(name, op, tuple(shape), dtype, n, tf, path, forced, batch, normalize, weights, kind, seed)
    assert name not in cases, name
    cases[name] = c


def _tf_for(op, i):
    return {"frequency": FREQ_TF[i % 3], "spatial": SPATIAL_TF[i % 4], "iq": None}[op]


def one_hot_classes(sx):
    """(name, l) of the stored column classes of the half spectrum that exist for `sx`."""
    out = [("onehot_l0", 0)]
    if sx // 2 >= 2:
        out.append(("onehot_inner", 1))
    if sx % 2 == 1 and sx > 1:
        out.append(("onehot_last", sx // 2))
    if sx % 2 == 0:
        out.append(("onehot_half", sx // 2))
    return out


def _build():
    cases = {}
    # every small shape on both paths, dtype and transfer function rotating with the shape
    for i, shape in enumerate(SMALL):
        for j, op in enumerate(OPS):
            for path in (0, 1):
                _make(cases, "shape", op, shape, DTYPES[(i + 2 * j) % 6], _tf_for(op, i + j), path, normalize=bool((i + j) % 2),
                      seed=100 + i)
    # all six dtypes in both domains and for image quality, on both paths
    for shape in ((7, 9), (60, 60)):
        for i, dtype in enumerate(DTYPES):
            for j, op in enumerate(OPS):
                for path in (0, 1):
                    _make(cases, "dtype", op, shape, dtype, _tf_for(op, i + j + 1), path, normalize=bool(i % 2), seed=200 + i)
    # float64 values that are not float32 values: the narrowing is visible
    for op in OPS:
        for path in (0, 1):
            _make(cases, "narrow", op, (6, 7), "float64", _tf_for(op, 0), path, kind="thirds", seed=300)
    # long axes, several workgroups per pattern and several partial sums on path 1
    for i, shape in enumerate(WIDE):
        for j, op in enumerate(OPS):
            for path in (0, 1):
                _make(cases, "wide", op, shape, DTYPES[(3 * i + j) % 6], _tf_for(op, i + j), path, normalize=bool(j % 2),
                      seed=400 + i)
    # outputs that depend on the order of a path's f64 sums, so that a run shows which path it took.  The filter: +2^60
    # and -2^60 next to ordinary pixels cancel inside one thread's quad on path 0 and swallow the pixels between them
    # on path 1, so the means differ; a transfer function on the column l = 0 alone keeps the spikes' spectrum out of
    # the result.  Image quality: weights of +2^50 and -2^50 on the conjugate pair (1, 0), (sy - 1, 0).
    for shape, dtype in (((60, 60), "float32"), ((17, 300), "float64")):
        for path in (0, 1):
            _make(cases, "cancel", "frequency", shape, dtype, "column0", path, n=3, kind="cancel", seed=450)
            _make(cases, "cancel", "iq", shape, dtype, None, path, n=3, weights=True, kind="cancel_weights", seed=451)
    _make(cases, "cancel", "frequency", (17, 300), "float32", "column0", 1, n=7, batch=3, kind="cancel", seed=452)
    _make(cases, "cancel", "iq", (17, 300), "float32", None, 1, n=7, batch=3, weights=True, normalize=False,
          kind="cancel_weights", seed=453)
    # path 0 just under the LDS cap (more than 64 KiB of dynamic LDS)
    for j, op in enumerate(OPS):
        _make(cases, "large", op, (128, 96), DTYPES[2 * j], _tf_for(op, j), 0, seed=500)
    # the natural boundary, unforced
    for op, first in BOUNDARY.items():
        tf = {"frequency": "lowhigh", "spatial": "sobel", "iq": None}[op]
        _make(cases, "last0", op, (first - 1, first - 1), "uint8", tf, 0, n=1, seed=600)
        _make(cases, "first1", op, (first, first), "uint8", tf, 1, n=2, seed=601)
    # one-hot transfer functions, one per stored column class
    for shape in ((5, 8), (8, 5), (60, 60), (61, 59)):
        for tf, _ in one_hot_classes(shape[1]):
            for path in (0, 1):
                _make(cases, "onehot", "frequency", shape, "float32", tf, path, seed=700)
    # a second (and a short third) workspace batch
    for i, shape in enumerate(((12, 10), (17, 300))):
        for j, op in enumerate(OPS):
            _make(cases, "batch", op, shape, DTYPES[(4 + i + 3 * j) % 6], _tf_for(op, i), 1, n=7, batch=3,
                  normalize=bool(i), seed=800 + i)
    # degenerate patterns inside a healthy stack, in the middle of a batch and at its end
    for shape in ((7, 9), (60, 60)):
        for dtype in ("float32", "uint8"):
            for j, op in enumerate(OPS):
                _make(cases, "degenerate", op, shape, dtype, _tf_for(op, j), 0, n=8, kind="degenerate", seed=900)
                _make(cases, "degenerate", op, shape, dtype, _tf_for(op, j), 1, n=8, batch=3, kind="degenerate", seed=900)
        # the filtered result is constant: a table and a kernel of zeros.  (A one-hot table at a frequency the pattern
        # does not contain leaves round-off, not a constant: the table's float32 sin(pi) is 1.2e-16, not 0.)
        for op, tf in (("frequency", "zero"), ("spatial", "zero_k")):
            for path in (0, 1):
                _make(cases, "constant", op, shape, "float32", tf, path, kind="constant", seed=950)
                _make(cases, "constant", op, shape, "int16", tf, path, kind="constant", seed=951)
    # image quality without normalization of a degenerate stack, and with explicit weights and inertia_max
    for path in (0, 1):
        _make(cases, "degenerate", "iq", (7, 9), "float32", None, path, n=8, batch=3 if path else None, normalize=False,
              kind="degenerate", seed=900)
        _make(cases, "weights", "iq", (61, 59), "float32", None, path, n=3, weights=True, seed=960)
        _make(cases, "weights", "iq", (6, 7), "int16", None, path, n=3, weights=True, normalize=False, seed=961)
    # the stacks of the stored fixtures (tests/golden/fft_filter.npz, image_quality.npz)
    ff = np.load(os.path.join(GOLDEN, "fft_filter.npz"))
    iq = np.load(os.path.join(GOLDEN, "image_quality.npz"))
    for i, shape in enumerate(s for s in _iq_inputs.SHAPES if s[0] * s[1] <= 128 * 96):
        for j, dtype in enumerate(_iq_inputs.DTYPES):
            key = f"rand__{shape[0]}x{shape[1]}__{dtype}"
            tf = str(ff[key + "__case"])
            op = ff_cases.CASES[tf][0]
            for path in ((0, 1) if shape != (128, 96) else (0,)):
                _make(cases, "fixture", op, shape, dtype, tf, path, n=ff_cases.N_STORED, kind="fixture",
                      seed=int(ff[key + "__seed"]))
                _make(cases, "fixture", "iq", shape, dtype, None, path, n=4, normalize=bool((i + j) % 2), kind="fixture",
                      seed=int(iq[key + "__seed"]))
    return cases


CASES = _build()
NAMES = list(CASES)
MISALIGNED_SHAPES = [(8, 8), (60, 60)]  # handed over one element behind a 256-byte boundary


def find(tag, op, shape, path, dtype=None, tf=None):
    """The name of the one case with this tag, operation, shape and path (and dtype and transfer function, if given)."""
    hits = [c.name for c in CASES.values() if c.name.startswith(tag + "-") and c.op == op and c.shape == tuple(shape)
            and c.path == path and dtype in (None, c.dtype) and tf in (None, c.tf)]
    assert len(hits) == 1, (tag, op, shape, path, dtype, tf, hits)
    return hits[0]


def fixture_key(c):
    """The key of the stored reference result of a fixture case."""
    assert c.kind == "fixture"
    key = f"rand__{c.shape[0]}x{c.shape[1]}__{c.dtype}"
    return key if c.op != "iq" else f"{key}__norm{int(c.normalize)}"


# ---- inputs -----------------------------------------------------------------------------------------------------------
def hash_stack(shape, dtype, n, seed):
    """`n` patterns of tests/_iq_inputs.py's integer hash in any of the six dtypes.  Signed integers cover both signs;
    floats span [-300, 700) and hold a few exact zeros."""
    base = {"uint8": "uint8", "int8": "uint8", "uint16": "uint16", "int16": "uint16"}.get(dtype, "float32")
    parts, have = [], 0
    while have < n:
        parts.append(_iq_inputs.stack(shape, base, seed + 7919 * len(parts)))
        have += len(parts[-1])
    a = np.concatenate(parts)[:n]
    if dtype == "int8":
        return (a.astype(np.int16) - 128).astype(np.int8)
    if dtype == "int16":
        return (a.astype(np.int32) - 32768).astype(np.int16)
    if base == "float32":
        a = a.copy()
        a[:, 0, 0] = 0
        a[:, -1, -1] = 0
        a[:, a.shape[1] // 2, a.shape[2] // 2] = -0.0
    return a.astype(dtype)


@functools.lru_cache(maxsize=None)
def stack(name):
    c = CASES[name]
    if c.kind == "fixture":
        return _iq_inputs.stack(c.shape, c.dtype, c.seed)[: c.n]
    a = hash_stack(c.shape, c.dtype, c.n, c.seed)
    if c.kind == "thirds":
        a = a / 3.0
        assert a.dtype == np.float64 and np.any(a != a.astype(np.float32))
    if c.kind == "cancel":
        a = a.copy()
        a[:, 0, 0] = 2.0 ** 60
        a[:, 0, 1] = -(2.0 ** 60)
    if c.kind == "degenerate":
        # healthy 0, 3, 6; with a batch cap of 3: 1 in the middle of a batch, 2 and 5 at its end, 4 in the middle, 7 at
        # the end of the short last batch
        a = a.copy()
        a[1] = 0
        a[2] = 77
        if a.dtype.kind == "f":
            a[4, a.shape[1] // 2, a.shape[2] // 3] = np.nan
            a[5, 0, 0] = np.inf
            a[7, -1, -1] = -np.inf
        else:
            a[4] = a[4, 0, 0]
            a[5] = 0
            a[7] = 255
    a.setflags(write=False)
    return a


def transfer(name):
    """(transfer function or kernel, shift) of a filter case, what EBSD.fft_filter would be given."""
    c = CASES[name]
    sy, sx = c.shape
    if c.tf in ff_cases.CASES:
        _, shift, build = ff_cases.CASES[c.tf]
        return build(c.shape, ff_cases.OurFunctions()), shift
    if c.tf == "zero":
        return np.zeros(c.shape), False
    if c.tf == "column0":
        h = np.zeros(c.shape)
        h[:, 0] = 1 + 0.1 * np.arange(sy)
        return h, False
    if c.tf == "zero_k":
        return np.zeros((3, 3)), False
    if c.tf == "one":
        return np.array([[1.5]]), False
    # one-hot in the full spectrum at (k, l): the fold leaves one non-zero entry of the half spectrum, or for a
    # self-mirrored column with a k that is not its own mirror the pair (k, l), (-k, l)
    l = dict(one_hot_classes(sx))[c.tf]
    self_mirrored = l == 0 or 2 * l == sx
    k = sy // 2 if (self_mirrored and sy % 2 == 0) else min(1, sy - 1)
    h = np.zeros(c.shape)
    h[k, l] = 1.0
    return h, False


def table(name):
    """(domain code, table) of Context.fft_filter for a filter case."""
    from kikuchipy_amd.pattern._pattern import fft_filter_table

    c = CASES[name]
    tf, shift = transfer(name)
    return fft_filter_table(tf, c.op, shift, c.shape)


def iq_arguments(name):
    """(weights or None, inertia_max or 0) of an image-quality case: explicit ones are not point-symmetric."""
    c = CASES[name]
    if not c.weights:
        return None, 0.0
    k, l = np.mgrid[: c.shape[0], : c.shape[1]]
    w = ((5 * k + 3 * l) % 13 + 0.25 * k + 0.125 * l + 1.0).astype(np.float64)
    if c.kind == "cancel_weights":
        w[1, 0], w[c.shape[0] - 1, 0] = 2.0 ** 50, -(2.0 ** 50)
    return w, 7.3125


@functools.lru_cache(maxsize=None)
def expected(name, wrong=None):
    """(result, stages) of the restatement of a case on the path and with the batch cap it claims."""
    c = CASES[name]
    stages = {}
    if c.op == "iq":
        w, imax = iq_arguments(name)
        out = R.image_quality(stack(name), c.normalize, c.path, w, imax, wrong=wrong, batch=c.batch, stages=stages)
    else:
        out = R.fft_filter(stack(name), table(name)[1], c.op, c.path, wrong=wrong, batch=c.batch, stages=stages)
    out.setflags(write=False)
    return out, stages
