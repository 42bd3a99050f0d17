"""Adaptive histogram equalization restated in NumPy from the steps of DESIGN.md §12 (scikit-image 0.18.3's
equalize_adapthist, then kikuchipy's rescale_intensity to the dtype's range, as NumPy 1.26 evaluates them), every
dtype explicit, so that it gives the same bits on any NumPy.  Test infrastructure: tests/test_host_clahe.py pins it to
the reference's fixture, tests/test_gpu_clahe.py compares the GPU with it where the fixture has no entry."""

import numpy as np

LEVELS = 16384  # 2**14 grey levels
DTYPE_RANGE = {np.uint8: (0, 255), np.int8: (-128, 127), np.uint16: (0, 65535), np.int16: (-32768, 32767),
               np.float32: (-1, 1), np.float64: (-1, 1)}


def astype(y, dtype):
    """ndarray.astype(dtype) of float values on x86-64: integer dtypes truncate to int32 (NaN and values outside int32
    give INT32_MIN) and keep the low bits."""
    dt = np.dtype(dtype)
    y = np.asarray(y)
    if dt.kind == "f":
        return y.astype(dt)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(y) & (y >= -2147483648.0) & (y < 2147483648.0)
        i = np.where(ok, np.trunc(np.where(ok, y, 0)), -2147483648.0).astype(np.int64)
    bits = 8 * dt.itemsize
    u = i & ((1 << bits) - 1)
    if dt.kind == "i":
        u = np.where(u >= 1 << (bits - 1), u - (1 << bits), u)
    return u.astype(dt)


def to_uint16(p):
    """img_as_uint (scikit-image 0.18.3) of one pattern."""
    dt = p.dtype
    if dt == np.uint8:
        return p.astype(np.uint16) * np.uint16(257)
    if dt == np.uint16:
        return p.copy()
    if dt == np.int8:  # 7 -> 16 bits through 21: x * (2**21 - 1) // (2**7 - 1), floor-divided by 2**5
        return np.maximum((p.astype(np.int32) * 16513) // 32, 0).astype(np.uint16)
    if dt == np.int16:  # 15 -> 16 bits through 30
        return np.maximum((p.astype(np.int32) * 32769) // 16384, 0).astype(np.uint16)
    y = np.rint(p * dt.type(65535))  # in the pattern's float type
    y = np.minimum(np.maximum(y, dt.type(0)), dt.type(65535))  # NaN stays NaN
    return astype(y, np.uint16)


def float_range_ok(p):
    """img_as_uint's check for a float pattern: skipped when min / max are NaN."""
    if p.dtype.kind != "f":
        return True
    mn, mx = p.min(), p.max()
    return not (mn < -1.0 or mx > 1.0)


def to_14bit(u):
    mn, mx = int(u.min()), int(u.max())
    if mn == mx:
        return np.minimum(u, LEVELS - 1).astype(np.uint16)
    t = (u.astype(np.float64) - float(mn)) / (float(mx) - float(mn))
    return np.rint(t * float(LEVELS - 1) + 0.0).astype(np.uint16)  # rint: half to even, as np.round


def reflect(j, n):
    """numpy's 'reflect' padding as an index map: detector index of (unpadded) coordinate j >= 0, any distance."""
    j = np.asarray(j, dtype=np.int64)
    if n == 1:
        return np.zeros_like(j)
    m = j % (2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def clip_histogram(h, clim):
    """The reference's clip and redistribution, integer-exact, on one histogram."""
    h = np.array(h, dtype=np.int64)
    over = h > clim
    n = int((h[over] - clim).sum())
    h[over] = clim
    incr = n // h.size
    upper = clim - incr
    low = h < upper
    n -= int(low.sum()) * incr
    h[low] += incr
    mid = (h >= upper) & (h < clim)  # after the low bins were raised
    n += int((h[mid] - clim).sum())
    h[mid] = clim
    pos = np.arange(h.size)
    while n > 0:
        before = n
        for index in range(h.size):
            under = h < clim
            step = max(1, int(under.sum()) // n)
            take = under & (pos >= index) & ((pos - index) % step == 0)
            h[take] += 1
            n -= int(take.sum())
            if n <= 0:
                break
        if before == n:
            break
    return h


def clahe_14bit(v, ky, kx, clim, nbins):
    """The equalized 14-bit pattern (uint16) of a 14-bit pattern `v`."""
    sy, sx = v.shape
    bins = v.astype(np.int64) // (1 + LEVELS // nbins)
    nty, ntx = -(-sy // ky), -(-sx // kx)
    ry, rx = reflect(np.arange(nty * ky), sy), reflect(np.arange(ntx * kx), sx)
    region = bins[ry][:, rx].reshape(nty, ky, ntx, kx).transpose(0, 2, 1, 3).reshape(nty * ntx, ky * kx)
    idx = region + (np.arange(nty * ntx) * nbins)[:, None]
    hist = np.bincount(idx.ravel(), minlength=nty * ntx * nbins).reshape(nty * ntx, nbins).astype(np.int64)
    kk = ky * kx
    if clim < kk:
        hist = np.stack([clip_histogram(h, clim) for h in hist])
    scale = float(LEVELS - 1) / float(kk)
    lut = np.minimum(np.trunc(np.cumsum(hist, axis=1).astype(np.float64) * scale), float(LEVELS - 1))
    lut = lut.astype(np.int64).reshape(nty, ntx, nbins)
    # interpolation blocks of the padded image and the weights r / k, 1 - r / k
    py, px = np.arange(sy) + ky // 2, np.arange(sx) + kx // 2
    by, bx = py // ky, px // kx
    wy1, wx1 = (np.arange(ky) / ky)[py % ky], (np.arange(kx) / kx)[px % kx]
    ty = [np.clip(by - 1, 0, nty - 1), np.clip(by, 0, nty - 1)]
    tx = [np.clip(bx - 1, 0, ntx - 1), np.clip(bx, 0, ntx - 1)]
    wy = [1.0 - wy1, wy1]
    wx = [1.0 - wx1, wx1]
    acc = np.zeros((sy, sx), np.float32)
    for ey, ex in ((0, 0), (0, 1), (1, 0), (1, 1)):
        mapped = lut[ty[ey][:, None], tx[ex][None, :], bins].astype(np.float64)
        w = wx[ex][None, :] * wy[ey][:, None]
        acc = acc + (mapped * w).astype(np.float32)
    return acc.astype(np.uint16)


def final(e, dtype):
    """img_as_float, scikit-image's rescale to [0, 1], kikuchipy's rescale to the dtype's range, the cast."""
    x = e.astype(np.float64) * (1.0 / 65535)
    a, b = x.min(), x.max()
    x2 = ((x - a) / (b - a)) * 1.0 + 0.0 if a != b else x.copy()
    m, mx = x2.min(), x2.max()
    omin, omax = DTYPE_RANGE[np.dtype(dtype).type]
    with np.errstate(invalid="ignore", divide="ignore"):
        y = ((x2 - m) / float(mx - m)) * float(omax - omin) + float(omin)
    return astype(y, dtype)


def clip_count(clip_limit, ky, kx):
    kk = ky * kx
    return int(np.clip(clip_limit * kk, 1, None)) if clip_limit > 0 else kk


def equalize(p, ky, kx, clip_limit=0, nbins=128):
    """One pattern with a (ky, kx) kernel."""
    v = to_14bit(to_uint16(p))
    return final(clahe_14bit(v, ky, kx, clip_count(clip_limit, ky, kx), nbins), p.dtype)


def ebsd_kernel(kernel_size, sig_shape):
    sy, sx = sig_shape
    if kernel_size is None:
        return sx // 4, sy // 4
    if np.isscalar(kernel_size):
        return int(kernel_size), int(kernel_size)
    return int(kernel_size[0]), int(kernel_size[1])


def ebsd_equalize(stack, kernel_size=None, clip_limit=0, nbins=128):
    """EBSD.adaptive_histogram_equalization on a stack (..., sy, sx)."""
    stack = np.asarray(stack)
    ky, kx = ebsd_kernel(kernel_size, stack.shape[-2:])
    flat = stack.reshape((-1,) + stack.shape[-2:])
    return np.stack([equalize(p, ky, kx, clip_limit, nbins) for p in flat]).reshape(stack.shape)
