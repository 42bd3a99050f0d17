"""NumPy restatement of what the background-removal kernels of csrc/preproc.hip compute - static -> truncate -> dynamic ->
truncate - bit for bit, pinned to the reference's results (tests/golden/preproc.npz, oracle/kpdi_oracle.py) by
tests/test_host_preproc.py and compared exactly with every kernel form by tests/test_gpu_preproc_kernels.py.

Static step: the reference's remove_static_background (pattern/_pattern.py:392-435) as its py_func evaluates it under
NumPy - float32 throughout, IEEE division, np.min / np.max (NaN propagates), `.astype` on x86-64.

Dynamic step (pattern/_pattern.py:438-481), in the kernel's order and precision:
  1. the pattern cast to float32;
  2. correlated along the rows axis with the window of `taps()`: per output, acc = fma(w[u], v, acc) in float64 in
     ascending tap order from acc = 0, rounded to float32;
  3. the same along the columns axis, rounded to float32: the background b;
  4. y = x - b or x / b in float32;
  5. np.min / np.max of y (NaN propagates);
  6. ((y - mn) / f32(mx - mn)) * f32(omax - omin) + f32(omin), every operation rounded to float32;
  7. `.astype(dtype)` as NumPy casts on x86-64 (`astype` of tests/_downsample_restate.py).
Boundary: edge replication ("frequency": the Barnes FFT filter's pad) or SciPy's 'reflect' ("spatial"); the window may be
longer than the detector, in 'reflect' by several periods.

Degenerate patterns follow from the same arithmetic, as in the reference: a NaN anywhere in y makes mn and mx NaN and
with them every pixel; a constant y is 0 / 0 = NaN on every pixel; NaN is 0 in the integer dtypes and stays NaN in the
float dtypes.  A lone +inf in y (x / 0 with x > 0) makes the range inf: the finite pixels become omin, the inf pixel NaN.
ONE EXCEPTION: a constant pattern under the "frequency" filter.  The reference's float32 FFT returns the constant plus
its own round-off, which the rescale then stretches over the whole output range (the oracle gives 0, 127 and 255 on a
constant uint8 pattern); the correlation returns the constant exactly, so this restatement - and the kernels - give the
0 / 0 result: all 0 (integers) or all NaN (floats).

Measured distance to the reference (tests/test_host_preproc.py prints the figures, `pytest -s`):
  static only                               equal, every case and dtype
  dynamic, "spatial"                        equal on the golden Ni cases and on seeded patterns of uint8, int8, uint16,
                                            int16 (SciPy's float32-stored passes and symmetric order fall on the same
                                            grey levels)
  dynamic, "frequency", uint8 (golden Ni)   <= 1 level on <= 1.9e-4 of the pixels (contract: 1e-3); static then
                                            dynamic: 3.1e-5
  dynamic, "frequency", uint8 / int8 noise  <= 1 level on <= 3.5e-5 of the pixels, 8 x 60 x 60 (contract: 2e-3)
  dynamic, "frequency", uint16 / int16      <= 1 level on <= 3.1e-3 of the pixels of seeded noise (8 x 60 x 60, strictly
                                            positive under "divide") and on 1.21e-2 of the golden uint16 Ni patterns;
                                            asserted at twice each figure
  dynamic, "frequency", float32 / float64   <= 8.4e-7 on seeded values up to 1000 (asserted: the suite's 2e-4)
"""

import math
import struct

import numpy as np

from _downsample_restate import DTYPE_RANGE, astype

CONV_R = 8  # csrc/kernels.h: zeros on either side of the uploaded taps (CONV_R - 1 of them)


def taps(filter_domain, std, truncate=4.0):
    """(taps, centre, reflect) as gaussian_taps of csrc/pattern_ops.hip builds them: the same expressions in the same
    order on Python floats, with math.exp - the C library's exp the host code calls (NumPy's vector exp may differ from
    it in the last bit)."""
    if filter_domain == "frequency":
        n = int(truncate * std)
        if n < 1:
            raise ValueError(f"Gaussian window of int(truncate*std) = {n} samples")
        w = []
        for i in range(n):
            x = i - (n - 1) / 2.0
            w.append(math.exp(-0.5 * (x / std) * (x / std)))
        centre, reflect = n - 1 - (n - 1) // 2, False
    elif filter_domain == "spatial":
        r = int(truncate * std + 0.5)
        w = []
        for i in range(2 * r + 1):
            x = float(i - r)
            w.append(math.exp(-0.5 / (std * std) * x * x))
        centre, reflect = r, True
    else:
        raise ValueError(f"{filter_domain} must be either of ['frequency', 'spatial']")
    total = 0.0
    for t in w:
        total += t
    return np.array([t / total for t in w], dtype=np.float64), centre, reflect


def taps_padded(filter_domain, std, truncate=4.0):
    """The array the kernels read (upload_taps): CONV_R - 1 zeros, the taps, CONV_R - 1 zeros.  The unrolled forms
    multiply by the padding zeros too; 0 * v added to the accumulator changes nothing for a finite v."""
    w, centre, reflect = taps(filter_domain, std, truncate)
    return np.concatenate([np.zeros(CONV_R - 1), w, np.zeros(CONV_R - 1)]), centre, reflect


def source_index(i, n, reflect):
    """wrap_index of csrc/preproc.hip: clamp, or scipy.ndimage 'reflect' (d c b a | a b c d | d c b a) at any distance."""
    i = np.asarray(i)
    if not reflect:
        return np.clip(i, 0, n - 1)
    i = np.mod(i, 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def split_tap(w):
    """w = hi + lo with `hi` the top 29 bits of the significand: hi * v and lo * v are exact for a float32 v."""
    hi = struct.unpack("<d", struct.pack("<Q", struct.unpack("<Q", struct.pack("<d", w))[0] & ~((1 << 24) - 1)))[0]
    return hi, w - hi


def fma_f32(w, v, acc):
    """fma(w, v, acc) in float64, correctly rounded, for a `v` that is a float32 value: both partial products are exact
    and math.fsum rounds the exact sum of the three once."""
    hi, lo = split_tap(float(w))
    v = float(v)
    return math.fsum((float(acc), hi * v, lo * v))


def correlate_fma(x, w, centre, reflect, axis, window_offset=0, drop_tap=None):
    """float64 correlation of the float32 array `x` (..., sy, sx) along `axis` (-2 or -1) with the kernel's fused
    accumulation, rounded to float32.  Evaluated with a separately rounded multiply and add, then every output whose
    float32 rounding the accumulated float64 error could move is redone with `fma_f32`.
    `window_offset`, `drop_tap`: the planted errors of tests/test_host_preproc.py (centre off by one, a tap dropped)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and axis in (-2, -1)
    n = x.shape[axis]
    w = np.asarray(w, dtype=np.float64)
    use = [u for u in range(len(w)) if u != drop_tap]
    src = [source_index(np.arange(n) + u - centre + window_offset, n, reflect) for u in range(len(w))]
    xd = x.astype(np.float64)
    acc = np.zeros(x.shape, dtype=np.float64)
    mag = np.zeros(x.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for u in use:
            v = np.take(xd, src[u], axis=axis)
            acc = acc + w[u] * v
            mag = mag + np.abs(w[u]) * np.abs(v)
        # each of the two evaluations is within (n + 1) u sum|w v| (1 + O(u)) of the exact sum, u = 2^-53
        bound = 4.0 * (len(use) + 2) * 2.0 ** -53 * mag
        out = acc.astype(np.float32)
        redo = np.isfinite(acc) & ((acc - bound).astype(np.float32) != (acc + bound).astype(np.float32))
    if redo.any():
        xm = np.moveaxis(x, axis, -1)
        om = np.moveaxis(out, axis, -1)  # a view: writes land in `out`
        for idx in zip(*np.nonzero(np.moveaxis(redo, axis, -1))):
            line = xm[idx[:-1]]
            a = 0.0
            for u in use:
                a = fma_f32(w[u], line[src[u][idx[-1]]], a)
            om[idx] = np.float32(a)
    return out


def rescale(y, dtype):
    """remove-background's rescale to the range of `dtype` and the cast: steps 5 - 7."""
    omin, omax = DTYPE_RANGE[np.dtype(dtype).type]
    assert y.dtype == np.float32
    with np.errstate(all="ignore"):
        mn, mx = np.min(y), np.max(y)  # NaN propagates
        r = (y - mn) / np.float32(mx - mn)
        r = r * np.float32(omax - omin) + np.float32(omin)
    assert r.dtype == np.float32
    return astype(r, dtype)


def remove_static(pattern, bg, operation="subtract", scale_bg=False):
    """One pattern (sy, sx); `bg`: the static background, cast to float32 as the API takes it."""
    x = astype(pattern, np.float32)
    b = np.asarray(bg).astype(np.float32)
    with np.errstate(all="ignore"):
        if scale_bg:
            bmin, bmax, pmin, pmax = np.min(b), np.max(b), np.min(x), np.max(x)
            b = ((b - bmin) / np.float32(bmax - bmin)) * np.float32(pmax - pmin) + pmin
        y = x - b if operation == "subtract" else x / b
    return rescale(y.astype(np.float32), pattern.dtype)


def remove_dynamic(pattern, operation="subtract", filter_domain="frequency", std=None, truncate=4.0, *, window_offset=0,
                   drop_tap=None, swap_boundary=False, same_axis=False):
    """One pattern (sy, sx).  The keyword-only arguments plant the errors of tests/test_host_preproc.py."""
    if std is None or std <= 0:
        std = pattern.shape[-1] / 8.0
    w, centre, reflect = taps(filter_domain, std, truncate)
    if swap_boundary:
        reflect = not reflect
    x = astype(pattern, np.float32)
    t = correlate_fma(x, w, centre, reflect, -2, window_offset, drop_tap)
    b = correlate_fma(t, w, centre, reflect, -2 if same_axis else -1, window_offset, drop_tap)
    with np.errstate(all="ignore"):
        y = x - b if operation == "subtract" else x / b
    return rescale(y.astype(np.float32), pattern.dtype)


def preprocess(stack, bg=None, *, static=True, dynamic=True, operation="subtract", scale_bg=False,
               filter_domain="frequency", std=None, truncate=4.0, **planted):
    """static -> truncate -> dynamic -> truncate of every pattern of `stack` (..., sy, sx), in the patterns' dtype."""
    stack = np.asarray(stack)
    flat = stack.reshape((-1,) + stack.shape[-2:])
    out = np.empty_like(flat)
    for j, p in enumerate(flat):
        if static:
            p = remove_static(p, bg, operation, scale_bg)
        if dynamic:
            p = remove_dynamic(p, operation, filter_domain, std, truncate, **planted)
        out[j] = p
    return out.reshape(stack.shape)
