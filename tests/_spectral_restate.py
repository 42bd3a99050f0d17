"""The FFT filter (csrc/fftfilter.hip) and image quality (csrc/iq.hip) restated in the kernels' own arithmetic, NumPy
only: f32 `fmaf` chains in the kernels' order (csrc/pattern_dft.h), twiddles indexed by the exact integer (k n) mod N,
f64 sums in `block_reduce`'s order, the min / max rescale in f64 (frequency domain) or f32 (spatial domain).  Vectorised
over patterns and outputs, sequential along every reduction index, so a GPU result can be held to it bit for bit.

`path` is the kernel path (0: one workgroup per pattern in LDS, 1: workspace): the two differ in the order of the f64
sums only.  `stages`, a dict, receives the intermediates (the mean, X after the rows, G after the columns times the
table, the filtered f32 pattern, its minimum and maximum), so that a failing test can say what the restatement held.

`wrong=` makes one deliberate mistake, for tests/test_host_spectral.py to show that the cases can tell it apart:
  "self_twice"  the self-mirrored column 2 l == sx counted twice
  "last_once"   the last stored column of an odd sx counted once
  "twiddle_mod" twiddle index (k n) mod (N - 1)
  "no_fma"      a * b + c, rounded twice, in place of fmaf
  "mean_f64"    the mean left in f64
  "other_sum"   the f64 sums in the other path's order
  "batch_offset" with `batch`: pattern start + i reads pattern i
  "int8_as_uint8" int8 rescaled onto uint8's range"""

import math

import numpy as np

F32, F64 = np.float32, np.float64
THREADS = 256  # FF_THREADS = IQ_THREADS
DTYPE_RANGE = {"uint8": (0.0, 255.0), "int8": (-128.0, 127.0), "uint16": (0.0, 65535.0), "int16": (-32768.0, 32767.0),
               "float32": (-1.0, 1.0), "float64": (-1.0, 1.0)}


# ---- f32 arithmetic ---------------------------------------------------------------------------------------------------
def fma_f32(a, b, c):
    """Correctly rounded float32 fma(a, b, c) of float32 operands.  The product of two f32 values is exact in f64; the
    f64 sum with c is rounded, its TwoSum residual exact.  Rounding that sum to f32 is right unless it sits exactly on
    an f32 tie while the residual says the true value lies to one side: then the result moves to that side."""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a.astype(F64) * b.astype(F64)
        cc = c.astype(F64)
        s = p + cc
        t = s - p
        err = (p - (s - t)) + (cc - t)
        r = s.astype(F32)
        rd = r.astype(F64)
        d = s - rd  # exact
        nb = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
        tie = (d != 0) & ((s - rd) == (nb.astype(F64) - s))
        move = tie & (((err > 0) & (d > 0)) | ((err < 0) & (d < 0)))
        return np.where(move, nb, r).astype(F32)


def mul_add_f32(a, b, c):
    """a * b + c with both roundings (what -ffp-contract=off gives a plain expression)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) * np.asarray(b, F32) + np.asarray(c, F32)).astype(F32)


def _fma(wrong):
    return mul_add_f32 if wrong == "no_fma" else fma_f32


def twiddles(n):
    """(cos, sin)(2 pi j / n) as float32, one libm call per entry, as write_twiddles of csrc/pattern_ops.hip."""
    c = np.array([F32(math.cos(2.0 * math.pi * j / n)) for j in range(n)], F32)
    s = np.array([F32(math.sin(2.0 * math.pi * j / n)) for j in range(n)], F32)
    return c, s


def _index(k, x, n, wrong):
    """The twiddle index of frequency (or position) `k` at step `x`: (k x) mod n, as the kernels' wrapped `j += k`."""
    if wrong == "twiddle_mod" and n > 1:
        return (k * x) % (n - 1)
    return (k * x) % n


def half_cols(sx):
    return sx // 2 + 1


def column_count(sx, wrong=None):
    """How often each stored column l = 0 ... sx / 2 counts in the full spectrum: 1 for l = 0 and 2 l == sx, else 2."""
    l = np.arange(half_cols(sx))
    c = np.where((l == 0) | (2 * l == sx), 1.0, 2.0)
    if wrong == "self_twice":
        c[2 * l == sx] = 2.0
    if wrong == "last_once" and sx % 2 == 1 and sx > 1:
        c[-1] = 1.0
    return c


def row_dft(pat, mean, tw, wrong=None):
    """X(y, l) = sum_x (pat(y, x) - mean) e^{-2 pi i l x / sx}, l < sx / 2 + 1: (re, im), float32 (n, sy, h)."""
    fma = _fma(wrong)
    n, sy, sx = pat.shape
    cos, sin = tw
    l = np.arange(half_cols(sx))
    re = np.zeros((n, sy, len(l)), F32)
    im = np.zeros((n, sy, len(l)), F32)
    for x in range(sx):
        if wrong == "mean_f64":
            v = (pat[:, :, x].astype(F64) - np.asarray(mean, F64)[:, None]).astype(F32)[:, :, None]
        else:
            v = (pat[:, :, x] - np.asarray(mean, F32)[:, None]).astype(F32)[:, :, None]
        j = _index(l, x, sx, wrong)
        re = fma(v, cos[j], re)
        im = fma(-v, sin[j], im)
    return re, im


def col_dft(x, tw, inv, wrong=None):
    """sum_y x(y, l) e^{-+2 pi i k y / sy} for every k (inv: +): (re, im), float32 (n, sy, h)."""
    fma = _fma(wrong)
    xr, xi = x
    n, sy, h = xr.shape
    cos, sin = tw
    k = np.arange(sy)
    re = np.zeros((n, sy, h), F32)
    im = np.zeros((n, sy, h), F32)
    for y in range(sy):
        j = _index(k, y, sy, wrong)
        c = cos[j][None, :, None]
        sn = (sin[j] if inv else -sin[j])[None, :, None]
        ar, ai = xr[:, y, :][:, None, :], xi[:, y, :][:, None, :]
        re = fma(ar, c, fma(-ai, sn, re))
        im = fma(ai, c, fma(ar, sn, im))
    return re, im


def row_idft(y, tw, sx, wrong=None):
    """sum_l Re(Y(l) e^{2 pi i l x / sx}) over the stored columns: float32 (n, sy, sx)."""
    fma = _fma(wrong)
    yr, yi = y
    n, sy, h = yr.shape
    cos, sin = tw
    x = np.arange(sx)
    v = np.zeros((n, sy, sx), F32)
    for l in range(h):
        j = _index(x, l, sx, wrong)
        v = fma(yr[:, :, l][:, :, None], cos[j], fma(-yi[:, :, l][:, :, None], sin[j], v))
    return v


def cmul(a, b, wrong=None):
    """ff_cmul: (fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x)), the bare products rounded to float32."""
    fma = _fma(wrong)
    with np.errstate(all="ignore"):
        return fma(a[0], b[0], (-a[1] * b[1]).astype(F32)), fma(a[0], b[1], (a[1] * b[0]).astype(F32))


# ---- f64 sums ---------------------------------------------------------------------------------------------------------
def block_sum(values_per_thread):
    """block_reduce<RedSum> of csrc/pattern_dft.h over the last axis (a multiple of 64 threads): an xor butterfly
    32 ... 1 within each wave of 64, then, from 0, the waves' results in wave order."""
    t = np.asarray(values_per_thread, F64)
    t = t.reshape(t.shape[:-1] + (t.shape[-1] // 64, 64))
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            t = t + t[..., lanes ^ o]
        s = np.zeros(t.shape[:-2])
        for w in range(t.shape[-2]):
            s = s + t[..., w, 0]
    return s


def strided_sum(values, group=1):
    """Per-thread f64 sums of `values` (n, count), thread t taking the groups t, t + 256, ... of `group` consecutive
    values in turn (a short tail padded with zeros), then block_sum."""
    v = np.asarray(values, F64)
    n, count = v.shape
    per = THREADS * group
    rounds = -(-count // per)
    padded = np.zeros((n, rounds * per))
    padded[:, :count] = v
    padded = padded.reshape(n, rounds, THREADS, group)
    acc = np.zeros((n, THREADS))
    with np.errstate(all="ignore"):
        for r in range(rounds):
            for e in range(group):
                acc = acc + padded[:, r, :, e]
    return block_sum(acc)


def workgroup_sums(values):
    """Path 1 of image quality: one value per thread, block_sum per workgroup of 256, then the workgroups in order."""
    v = np.asarray(values, F64)
    n, count = v.shape
    blocks = -(-count // THREADS)
    padded = np.zeros((n, blocks * THREADS))
    padded[:, :count] = v
    part = block_sum(padded.reshape(n, blocks, THREADS))
    s = np.zeros(n)
    with np.errstate(all="ignore"):
        for b in range(blocks):
            s = s + part[:, b]
    return s


def _batch_view(stack, batch, wrong):
    if wrong == "batch_offset" and batch:
        return stack[np.arange(len(stack)) % batch]
    return stack


# ---- the FFT filter ---------------------------------------------------------------------------------------------------
def correlate(pat, taps):
    """ff_correlate: the correlation with clamped indices centred at (ty // 2, tx // 2), the kernel's columns v outside
    and its rows u inside, in f64 (every product of two f32 values is exact there), rounded to float32 at the end."""
    n, sy, sx = pat.shape
    w = np.asarray(taps).astype(F32).astype(F64)
    ty, tx = w.shape
    p = pat.astype(F64)
    acc = np.zeros((n, sy, sx))
    ys, xs = np.arange(sy), np.arange(sx)
    with np.errstate(all="ignore"):
        for v in range(tx):
            cols = p[:, :, np.clip(xs + v - tx // 2, 0, sx - 1)]
            for u in range(ty):
                acc = w[u, v] * cols[:, np.clip(ys + u - ty // 2, 0, sy - 1), :] + acc
        return acc.astype(F32)


def rescale(f, bad, dtype, freq, wrong=None):
    """FfRescale and ff_cast: per pattern ((V(v) - min) / (max - min)) * (hi - lo) + lo in V = f64 (frequency) or f32
    (spatial), truncated to integer dtypes; a degenerate pattern is NaN before the cast, 0 after it for integers."""
    dtype = np.dtype(dtype)
    lo, hi = DTYPE_RANGE["uint8" if (wrong == "int8_as_uint8" and dtype == np.int8) else dtype.name]
    V = F64 if freq else F32
    n = len(f)
    flat = f.reshape(n, -1)
    with np.errstate(all="ignore"):
        mn, mx = flat.min(axis=1).astype(F32), flat.max(axis=1).astype(F32)
        nan_case = np.asarray(bad, bool) | ~(mx > mn) | ~np.isfinite((mx - mn).astype(F32))
        imin = mn.astype(V)
        irange = mx.astype(V) - mn.astype(V)
        orange = V(F32(hi)) - V(F32(lo))
        v = ((flat.astype(V) - imin[:, None]) / irange[:, None]) * orange + V(F32(lo))
        v = np.where(nan_case[:, None], V(np.nan), v)
        if dtype.kind in "iu":
            v = np.trunc(np.where(np.isnan(v), V(0), v))
            if wrong == "int8_as_uint8" and dtype == np.int8:
                v = np.where(v > 127, v - 256, v)
        return v.astype(dtype).reshape(f.shape), mn, mx, nan_case


def fft_filter(stack, table, domain, path, wrong=None, batch=None, stages=None):
    """kpdi_fft_filter of a stack (n, sy, sx): `table` is the folded half spectrum (sy, sx // 2 + 1) complex
    (`domain` "frequency") or the real correlation kernel ("spatial").  Returns an array of the stack's dtype."""
    stack = _batch_view(np.asarray(stack), batch, wrong)
    n, sy, sx = stack.shape
    npix = sy * sx
    with np.errstate(all="ignore"):
        pat = stack.astype(F32)
    bad = ~np.isfinite(pat).reshape(n, -1).all(axis=1)
    order = path if wrong != "other_sum" else 1 - path
    s = strided_sum(pat.reshape(n, -1), 4 if order == 0 else 1)
    with np.errstate(all="ignore"):
        mean = s / npix if wrong == "mean_f64" else (s / npix).astype(F32)
    safe = np.where(bad[:, None, None], F32(0), pat)  # (a degenerate pattern's result is not read)
    safe_mean = np.where(bad, 0, mean)
    st = {"mean": mean, "sum": s}
    if domain == "frequency":
        t = np.asarray(table, np.complex128)
        assert t.shape == (sy, half_cols(sx)), t.shape
        scale = 1.0 / (float(sy) * float(sx))
        hs = ((t.real * scale).astype(F32)[None], (t.imag * scale).astype(F32)[None])
        twx, twy = twiddles(sx), twiddles(sy)
        x = row_dft(safe, safe_mean, twx, wrong)
        g = cmul(col_dft(x, twy, False, wrong), hs, wrong)
        y = col_dft(g, twy, True, wrong)
        c = column_count(sx, wrong).astype(F32)
        f = row_idft(((c * y[0]).astype(F32), (c * y[1]).astype(F32)), twx, sx, wrong)
        st.update(X=x, G=g)
    else:
        f = correlate(safe, table)
    out, mn, mx, nan_case = rescale(f, bad, stack.dtype, domain == "frequency", wrong)
    st.update(filtered=f, min=mn, max=mx, degenerate=nan_case)
    if stages is not None:
        stages.update(st)
    return out


# ---- image quality ----------------------------------------------------------------------------------------------------
def default_weights(sy, sx):
    """kpdi_image_quality's default weights: the reference's fft_frequency_vectors."""
    def line(n):
        i = np.arange(n)
        return np.where(i < n // 2, i + 1, i - n).astype(F64)

    return line(sy)[:, None] ** 2 + line(sx)[None, :] ** 2 - 1.0


def fold_weights(w):
    """W(k, l) = w(k, l) + w(-k, -l) for the stored columns whose mirror is not stored, else w(k, l)."""
    sy, sx = w.shape
    h = half_cols(sx)
    l = np.arange(h)
    self_mirrored = (l == 0) | (2 * l == sx)
    mirror = w[(-np.arange(sy)) % sy][:, (sx - l) % sx]
    return w[:, :h] + np.where(self_mirrored[None, :], 0.0, mirror)


def image_quality(stack, normalize, path, weights=None, inertia_max=None, wrong=None, batch=None, stages=None):
    """kpdi_image_quality of a stack (n, sy, sx): float32 (n,)."""
    stack = _batch_view(np.asarray(stack), batch, wrong)
    n, sy, sx = stack.shape
    npix, h = sy * sx, half_cols(sx)
    with np.errstate(all="ignore"):
        pat = stack.astype(F32)
    flat = pat.reshape(n, -1)
    bad = ~np.isfinite(flat).all(axis=1)
    with np.errstate(all="ignore"):
        degenerate = bad | (bool(normalize) & (flat.min(axis=1) == flat.max(axis=1)))
    s = strided_sum(flat)  # (stat_one takes single pixels t, t + 256, ... on both paths)
    with np.errstate(all="ignore"):
        mean = s / npix if wrong == "mean_f64" else (s / npix).astype(F32)
    w = default_weights(sy, sx) if weights is None else np.asarray(weights, F64)
    if inertia_max is None or inertia_max <= 0:
        total = 0.0
        for v in w.ravel():
            total += float(v)
        inertia_max = total / (float(sy) * float(sx))
    wf = fold_weights(w).ravel()
    safe = np.where(degenerate[:, None, None], F32(0), pat)
    x = row_dft(safe, np.where(degenerate, 0, mean), twiddles(sx), wrong)
    fr, fi = col_dft(x, twiddles(sy), False, wrong)
    with np.errstate(all="ignore"):
        mag = np.sqrt(((fr * fr).astype(F32) + (fi * fi).astype(F32)).astype(F32)).astype(F32)
        a = mag.astype(F64).reshape(n, -1)
        if not normalize:
            a[:, 0] = np.abs(s)
        cnt = np.tile(column_count(sx, wrong), sy)
        tw_, ts_ = wf[None, :] * a, cnt[None, :] * a
        order = path if wrong != "other_sum" else 1 - path
        if order == 0:
            sw, ss = strided_sum(tw_), strided_sum(ts_)
        else:
            sw, ss = workgroup_sums(tw_), workgroup_sums(ts_)
        q = (1.0 - (sw / ss) / float(inertia_max)).astype(F32)
    q = np.where(degenerate, F32(np.nan), q).astype(F32)
    if stages is not None:
        stages.update(mean=mean, sum=s, X=x, F=(fr, fi), magnitude=mag, sw=sw, ss=ss, degenerate=degenerate)
    return q
