"""The shapes the decomposition tests run on and a float64 NumPy restatement of what the GPU computes: centring with the
documented summation order of the means, the Gram matrix, `numpy.linalg.svd` of the centred matrix, the sign rule and the
model.  Shared by tests/test_host_decomposition.py and tests/test_gpu_decomposition.py; pure NumPy, no GPU.

The shapes make every tile edge of csrc/decomp.hip occur (64 x 64 output tiles, reduction stages of 16): K = 91 and 143
(two and three tiles per side, edges of 27 and 15), M = 48 (one partial tile, the transposed branch), a reduction of 2100
over a 35 x 35 output, and 9 patterns of 60 x 60 (a 9 x 9 Gram matrix over 3600 pixels)."""

import os

import numpy as np

from _spectral_restate import block_sum  # the workgroup reduction's order, restated once

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#        name: (navigation shape, pattern shape)
CASES = {
    "A": ((17, 19), (7, 13)),
    "B": ((17, 19), (11, 13)),
    "C": ((6, 8), (12, 20)),
    "D": ((2100,), (5, 7)),
    "E": ((9,), (60, 60)),
}
CENTRES = (None, "navigation", "signal")
TILE, KB, MEAN_ROWS, THREADS, MAX_SIDE = 64, 16, 256, 256, 8192  # csrc/decomp_plan.h


def dims(name):
    nav, sig = CASES[name]
    return int(np.prod(nav)), int(np.prod(sig))


def plan(m, k):
    """decomp_plan.h's dec_plan in Python: what the header must return."""
    transposed = k > m
    side, reduce_ = (m, k) if transposed else (k, m)
    if side > MAX_SIDE:
        return dict(ok=0, too_large=1, transposed=int(transposed), side=side)
    tiles = -(-side // TILE)
    return dict(ok=1, too_large=0, transposed=int(transposed), side=side, reduce=reduce_, tiles=tiles,
                edge=side % TILE or TILE, computed_tiles=tiles * (tiles + 1) // 2, steps=-(-reduce_ // KB),
                tail=reduce_ % KB or KB)


def integers(name, dtype, seed=0):
    """Seeded random integers over the whole range of `dtype` (uint8 / uint16), or, float32, integers below 2^12."""
    nav, sig = CASES[name]
    rng = np.random.default_rng([seed, ord(name)])
    if np.dtype(dtype).kind == "f":
        return rng.integers(-4096, 4096, nav + sig).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, int(info.max) + 1, nav + sig).astype(dtype)


def ni_patterns():
    """The nine Ni patterns of the fixtures, (9, 60, 60) uint8."""
    return np.load(os.path.join(ROOT, "tests", "golden", "preproc.npz"))["ni"].reshape(9, 60, 60)


def patterns(name, dtype, seed=1):
    """Patterns of case `name`: the Ni patterns for E, else seeded random ones with a smooth common part (so that the
    mean is not negligible); float dtypes hold non-integers."""
    nav, sig = CASES[name]
    if name == "E":
        p = ni_patterns().astype(np.float64)
    else:
        rng = np.random.default_rng([seed, ord(name)])
        yy, xx = np.mgrid[: sig[0], : sig[1]]
        p = 90.0 + 40.0 * np.cos(0.3 * yy + 0.2 * xx) + 50.0 * rng.random(nav + sig) + 20.0 * rng.random(nav + (1, 1))
    if np.dtype(dtype).kind == "f":
        return (p / 3.0).astype(dtype).reshape(nav + sig)
    return p.astype(dtype).reshape(nav + sig)


def low_rank_patterns(name, rank=12, seed=2):
    """sum_r 2^-r u_r v_r^T over `rank` orthonormal pairs (r = 1 ... rank) plus noise of 2^-20, as float32."""
    nav, sig = CASES[name]
    m, k = dims(name)
    rng = np.random.default_rng([seed, ord(name)])
    u = np.linalg.qr(rng.standard_normal((m, rank)))[0]
    v = np.linalg.qr(rng.standard_normal((k, rank)))[0]
    x = (u * 2.0 ** -np.arange(1, rank + 1)) @ v.T + 2.0 ** -20 * rng.standard_normal((m, k))
    return x.astype(np.float32).reshape(nav + sig)


def matrix(p):
    """(M, K) float64 of a stack."""
    return np.asarray(p).reshape((-1, p.shape[-2] * p.shape[-1])).astype(np.float64)


# ---- the means, in the order csrc/decomp.hip documents --------------------------------------------------------------
def mean_signal(x):
    """One mean per pattern: thread t of 256 adds pixels t, t + 256, ... in turn; an xor butterfly 32 ... 1 within each
    wave of 64; the four waves in order; / K."""
    m, k = x.shape
    rows = -(-k // THREADS)
    padded = np.zeros((m, rows * THREADS))
    padded[:, :k] = x
    padded = padded.reshape(m, rows, THREADS)
    t = np.zeros((m, THREADS))
    for r in range(rows):
        t = t + padded[:, r]
    return block_sum(t) / float(k)


def mean_navigation(x):
    """The mean pattern: per pixel the rows of each block of 256 patterns in turn, then the blocks in turn; / M."""
    m, k = x.shape
    s = np.zeros(k)
    for m0 in range(0, m, MEAN_ROWS):
        part = np.zeros(k)
        for r in range(m0, min(m0 + MEAN_ROWS, m)):
            part = part + x[r]
        s = s + part
    return s / float(m)


def centred(x, centre):
    """(Xc, mean): xc = double(x) - mean, rounded once."""
    if centre is None:
        return x, None
    if centre == "signal":
        mu = mean_signal(x)
        return x - mu[:, None], mu
    mu = mean_navigation(x)
    return x - mu[None, :], mu


def gram(xc):
    """(Gram matrix over the shorter side, transposed)."""
    m, k = xc.shape
    return (xc @ xc.T, True) if k > m else (xc.T @ xc, False)


def sign_rule(factors, loadings):
    """Each factor's entry of largest magnitude (the first on a tie) becomes positive; its loading follows."""
    for j in range(factors.shape[1]):
        i = int(np.argmax(np.abs(factors[:, j])))
        if factors[i, j] < 0:
            factors[:, j] = -factors[:, j]
            loadings[:, j] = -loadings[:, j]


def svd_results(xc, c):
    """(factors (K, c), loadings (M, c), explained variance of all min(M, K) components, singular values) from a direct
    SVD of the centred matrix; components with sigma^2 <= side 2^-52 sigma_1^2 are null: exactly zero."""
    m, k = xc.shape
    u, s, vt = np.linalg.svd(xc, full_matrices=False)
    factors = np.ascontiguousarray(vt[:c].T)
    loadings = u[:, :c] * s[:c]
    null = s[:c] ** 2 <= min(m, k) * 2.0 ** -52 * s[0] ** 2
    factors[:, null] = 0.0
    loadings[:, null] = 0.0
    sign_rule(factors, loadings)
    return factors, loadings, s ** 2 / m, s


def pick(a, components):
    """signals/util/_dask.py:319-324."""
    return a[:, components] if hasattr(components, "__iter__") else a[:, :components]


def model(factors, loadings, mean, centre, components=None, dtype_out=np.float32):
    """The model in float64 from factors / loadings cast to `dtype_out` first; the caller rounds it."""
    f = pick(factors.astype(dtype_out), components).astype(np.float64)
    lo = pick(loadings.astype(dtype_out), components).astype(np.float64)
    out = lo @ f.T
    if centre == "signal":
        out = out + mean[:, None]
    elif centre == "navigation":
        out = out + mean[None, :]
    return out


def edges_gap(lam, components, c_all):
    """The smallest eigenvalue gap at the edges of the chosen set of components: between a chosen component and an
    unchosen neighbour (`lam` descending, all eigenvalues; the component after the last computed one counts)."""
    chosen = set(range(c_all)[:components] if not hasattr(components, "__iter__") else components)
    gaps = []
    for j in chosen:
        for n in (j - 1, j + 1):
            if 0 <= n < len(lam) and n not in chosen:
                gaps.append(abs(lam[j] - lam[n]))
    return min(gaps) if gaps else np.inf


def gram_error(xc):
    """E = (M + side) 2^-52 || |Xc|^T |Xc| ||_2: what rounding may add to the Gram matrix, as a spectral norm."""
    m, k = xc.shape
    a = np.abs(xc)
    return (m + min(m, k)) * 2.0 ** -52 * np.linalg.norm(a.T @ a if k <= m else a @ a.T, 2)
