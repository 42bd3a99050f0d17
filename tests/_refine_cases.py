"""Case tables and float64 restatements for the two pieces of csrc/refine.hip every optimiser stands on: refine_prep_kernel
(through kpdi_refine_set_patterns / kpdi_refine_get_prepared) and refine_objective (through kpdi_refine_objective and,
inlined, the three device solvers).  Seeded, NumPy and the NumPy oracle only, no GPU.  tests/test_host_refine_cases.py
checks the tables against the oracle and shows that wrong variants of the restatement leave the tolerance;
tests/test_gpu_refine_kernels.py runs the tables through the kernels.

`prep64` PREDICTS THE BITS of a prepared pattern and its squared norm: float32 cast, optional rescale in float32 in the
kernel's order ((v - lo) / span * 2 + -1), mean = float32(float64(exact sum) / k), float32 subtraction, squared norm =
float64(float32(exact sum of squares)), exact = math.fsum.  The kernel sums in float64 in an order of its own, so the
builder only keeps inputs on which the order cannot show (`order_complaints`): the summed values are integers below 2^53
in total (integer dtypes without rescale) or multiples of 2^-40 whose absolute values sum to less than 2^12, so every
partial sum is exact; and the exact sum of squares is further than 1e-12 (relative) from every float32 rounding midpoint,
ten times what a float64 sum of 1000 positive terms can be off by.

`objective64` restates refine_objective: direction cosines for the PC, rotation, Lambert interpolation and the float32
cast of every simulated value from the oracle's helpers, then the three sums and var = s2 - s1^2 / k in float64 (exactly
rounded sums).  Its tolerance comes from itself: sum(|df/dsim_c| * ulp32(sim_c)), what the objective moves when every
simulated value is off by one float32 ulp in the worst direction (the kernel's float64 value before the cast differs
from NumPy's in the last bits, so a value next to a rounding boundary may fall either way), plus eps64 * k * s2 / var for
the cancellation in the one-pass variance.  8e-9 to 3e-7 on the cases here, median 6e-8, and up to 2e-5 on the 1 x 257
detector with the PC outside it, where the simulated pattern is nearly constant (s2 / var up to 9e4).

Every geometry case asserts its own premises while it is built: k >= 8, no rotated z within 1e-9 of 0 (a pixel in the
wrong hemisphere is then a bug, not rounding), s2 / var <= 1e6, and at least a tenth of the pixels in the smaller
hemisphere wherever TWO_HEMISPHERES says so."""
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import kpdi_oracle as ko

ORI, PC, ORI_PC = 0, 1, 2  # include/kpdi.h KPDI_REFINE_*
MODES = {"ori": ORI, "pc": PC, "ori_pc": ORI_PC}
EPS64 = float(np.finfo(np.float64).eps)
N_PATTERNS = 3
PATTERN_INDEX = (2, 0, 2, 1)  # out of order, one of them twice


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2**32)


# ---- master patterns: two different smooth hemispheres, odd and even side ------------------------------------------------
def _hemisphere(seed, n):
    """A dozen plane waves of up to three periods across the pattern, scaled into [-1, 1]."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:n, :n] / float(n)
    a = np.zeros((n, n))
    for _ in range(12):
        fy, fx = rng.uniform(-3, 3, 2)
        a += rng.uniform(0.3, 1) * np.cos(2 * np.pi * (fy * y + fx * x) + rng.uniform(0, 2 * np.pi))
    return (a / np.abs(a).max()).astype(np.float32)


@functools.lru_cache(maxsize=None)
def master(kind):
    n, seeds = {"odd": (41, (11, 12)), "even": (40, (13, 14))}[kind]
    upper, lower = _hemisphere(seeds[0], n), _hemisphere(seeds[1], n)
    assert np.abs(upper - lower).mean() > 0.2  # the hemispheres really differ
    return upper, lower


# detector -> sample, every detector angle non-zero
OM = np.ascontiguousarray(ko.sample_to_detector_matrix(70.0, 4.0, 7.0, 3.0).T)

PCS = {"mid": (0.45, 0.7, 0.55), "corner": (0.81, 0.22, 0.72), "outside": (-0.2, 1.3, 0.3), "near": (0.52, 0.58, 0.15)}
EULERS = {"Phi0": (1.1, 0.0, 0.7), "PhiPi": (0.4, np.pi - 1e-3, 2.0), "flip": (3.0, 1.0, 2.5), "plain": (0.3, 1.45, 5.1)}
assert ko.rotation_from_euler(3.0, 1.0, 2.5)[0] > 0 > np.cos(0.5) * np.cos(2.75)  # "flip" takes the q[0] < 0 branch

# ---- geometry cases -----------------------------------------------------------------------------------------------------
Geometry = namedtuple("Geometry", "name shape mask master")
GEOMETRIES = (
    Geometry("5x7", (5, 7), "none", "odd"),
    Geometry("7x5", (7, 5), "none", "even"),
    Geometry("16x16", (16, 16), "none", "odd"),
    Geometry("1x257", (1, 257), "none", "odd"),
    Geometry("12x20", (12, 20), "none", "odd"),
    Geometry("3x3", (3, 3), "none", "even"),
    Geometry("16x16-one-masked", (16, 16), "one", "odd"),  # k = 255
    Geometry("16x16-circular", (16, 16), "circular", "even"),
    Geometry("12x20-circular", (12, 20), "circular", "odd"),
    Geometry("7x5-circular", (7, 5), "circular", "odd"),
    Geometry("12x20-checkerboard", (12, 20), "checkerboard", "even"),
    Geometry("5x7-checkerboard", (5, 7), "checkerboard", "odd"),
    Geometry("1x257-checkerboard", (1, 257), "checkerboard", "even"),
    Geometry("12x20-row-and-last", (12, 20), "row+last", "odd"),
    Geometry("5x7-row-and-last", (5, 7), "row+last", "even"),  # k = 8
    # the transpose of 12x20-circular: same pixels and mask, other shape
    Geometry("20x12-circular-T", (20, 12), "circular-T", "odd"),
)
GEOMETRY = {g.name: g for g in GEOMETRIES}
assert len(GEOMETRY) == len(GEOMETRIES)

# (PC, Euler set) pairs at which EVERY geometry has at least a tenth of its pixels in the smaller hemisphere (a third or
# more on most); `build_geometry` asserts it.  Elsewhere the pixels lie in one hemisphere, or nearly.
TWO_HEMISPHERES = frozenset({("mid", "plain"), ("corner", "flip"), ("near", "flip"), ("near", "plain")})


def keep_mask(shape, kind):
    """True = the pixel is used (the reference's convention inside the solvers)."""
    nrows, ncols = shape
    if kind == "none":
        return np.ones(shape, bool)
    if kind == "circular":
        return ko.circular_window(shape).astype(bool)
    if kind == "circular-T":
        return np.ascontiguousarray(ko.circular_window(shape[::-1]).astype(bool).T)
    r, c = np.mgrid[:nrows, :ncols]
    if kind == "checkerboard":
        return (r + c) % 2 == 0
    if kind == "row+last":
        keep = r == min(1, nrows - 1)
        keep[-1, -1] = True
        return keep
    if kind == "one":
        keep = np.ones(shape, bool)
        keep[5, 9] = False
        return keep
    raise ValueError(kind)


# ---- the objective, restated --------------------------------------------------------------------------------------------
FAULTS = ("hemispheres swapped", "aspect = nrows / ncols", "no half-pixel offset", "row and column swapped in the mask map",
          "mask map strided by nrows")


def simulate(shape, keep, q, pc, mp, fault=None):
    """The float32 simulated values of the kept pixels for quaternion q and PC pc, and the rotated z of every pixel.
    _get_direction_cosines_for_fixed_pc + _project_single_pattern_from_master_pattern, formulas of the oracle."""
    nrows, ncols = shape
    pcx, pcy, pcz = (float(v) for v in pc)
    aspect = nrows / ncols if fault == "aspect = nrows / ncols" else ncols / nrows
    x_min, x_max = -aspect * (pcx / pcz), aspect * (1 - pcx) / pcz
    y_min, y_max = -(1 - pcy) / pcz, pcy / pcz
    x_scale, y_scale = (x_max - x_min) / ncols, (y_max - y_min) / nrows
    idx = np.flatnonzero(np.asarray(keep).ravel())
    rows, cols = idx // ncols, idx % ncols
    if fault == "row and column swapped in the mask map":
        rows, cols = cols, rows
    if fault == "mask map strided by nrows":
        rows, cols = idx // nrows, idx % nrows
    half = 0.0 if fault == "no half-pixel offset" else 0.5
    r_g = np.empty((idx.size, 3))
    r_g[:, 0] = ((x_min + cols * x_scale) + half * x_scale) * pcz
    r_g[:, 1] = ((y_max + rows * (-y_scale)) - half * y_scale) * pcz
    r_g[:, 2] = pcz
    r_g = r_g @ OM.T
    dc = r_g / np.sqrt(np.sum(r_g**2, axis=-1))[:, None]
    v = ko.rotate_vector(q, dc)
    upper, lower = mp
    npy, npx = upper.shape
    nii, nij, niip, nijp, di, dj, dim, djm = ko.lambert_interpolation_parameters(v, npx, npy, float((npx - 1) / 2))
    up = v[:, 2] >= 0
    if fault == "hemispheres swapped":
        up = ~up
    sim = np.empty(idx.size)
    for sel, m in ((up, upper), (~up, lower)):
        sim[sel] = (m[nii[sel], nij[sel]] * dim[sel] * djm[sel] + m[niip[sel], nij[sel]] * di[sel] * djm[sel]
                    + m[nii[sel], nijp[sel]] * dim[sel] * dj[sel] + m[niip[sel], nijp[sel]] * di[sel] * dj[sel])
    return sim.astype(np.float32), v[:, 2]


def ncc_terms(sim32, pat, sqn):
    """(objective, tolerance, s2 / var) from the float32 simulated values, a prepared pattern and its squared norm."""
    sim = sim32.astype(np.float64)
    k = sim.size
    s1 = math.fsum(sim.tolist())
    s2 = math.fsum((sim * sim).tolist())
    s3 = math.fsum((pat.astype(np.float64) * sim).tolist())
    var = s2 - s1 * s1 / k
    den = math.sqrt(sqn * var)
    f = 1.0 - s3 / den
    # df/dsim_c = -pat_c / den + s3 (sim_c - mean) / (den var)
    grad = -pat.astype(np.float64) / den + s3 * (sim - s1 / k) / (den * var)
    tol = float(np.sum(np.abs(grad) * np.spacing(np.abs(sim32)).astype(np.float64))) + EPS64 * k * s2 / var
    return f, tol, s2 / var


def objective64(shape, keep, q, pc, mp, pat, sqn, fault=None):
    sim32, _ = simulate(shape, keep, q, pc, mp, fault)
    return ncc_terms(sim32, pat, sqn)[:2]


# ---- the preparation, predicted -----------------------------------------------------------------------------------------
def _fsum(a):
    a = np.asarray(a, dtype=np.float64)
    return math.fsum(a.tolist()) if np.isfinite(a).all() else float(np.sum(a))


def prep64(kept, rescale):
    """kept: the raw kept pixels of one pattern, any dtype.  Returns (prepared float32 pattern, squared norm as float64).
    np.min / np.max carry a NaN on where the kernel's fminf / fmaxf skip it; the NaN pixel itself then makes the sum, the
    mean and with them every pixel NaN in the kernel, which is what comes out here (the "edges" rows)."""
    with np.errstate(all="ignore"):
        v = np.asarray(kept).astype(np.float32)
        if rescale:
            lo, hi = np.min(v), np.max(v)
            v = (v - lo) / np.float32(hi - lo) * np.float32(2) + np.float32(-1)
        mean = np.float32(np.float64(_fsum(v)) / np.float64(v.size))
        c = v - mean
        assert c.dtype == np.float32
        c64 = c.astype(np.float64)
        return c, np.float64(np.float32(_fsum(c64 * c64)))


def order_complaints(kept, rescale):
    """Why the bits prep64 predicts could depend on the order of the kernel's float64 sums: [] if they cannot."""
    raw = np.asarray(kept)
    v = raw.astype(np.float32)
    if rescale:
        v = (v - np.min(v)) / np.float32(np.max(v) - np.min(v)) * np.float32(2) + np.float32(-1)
    v64 = v.astype(np.float64)
    bad = []
    if raw.dtype.kind in "iu" and not rescale:
        if not (np.abs(v64).sum() < 2.0**53 and (v64 == np.rint(v64)).all()):
            bad.append("integers that do not sum exactly")
    else:
        if not (v64 * 2.0**40 == np.rint(v64 * 2.0**40)).all():
            bad.append("a summed value is no multiple of 2^-40")
        if not np.abs(v64).sum() < 2.0**12:
            bad.append("partial sums may reach 2^12")
    c, _ = prep64(raw, rescale)
    s2 = _fsum(c.astype(np.float64) ** 2)
    if s2 > 0:
        f = np.float32(s2)
        for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
            mid = (np.float64(f) + np.float64(other)) / 2
            if abs(s2 - mid) <= 1e-12 * s2:
                bad.append("the sum of squares lies at a float32 rounding midpoint")
    return bad


# ---- a geometry case, built ---------------------------------------------------------------------------------------------
Evaluation = namedtuple("Evaluation", "pc_name eu_name pc eu q sim32 f tol share min_abs_z s2_over_var")
BuiltGeometry = namedtuple("BuiltGeometry", "geom keep mask_out k raw pat sqn mp evals")


def experimental_patterns(g, keep, mp, rng):
    """Three uint8 patterns that look like the simulation at three of the Euler sets (PC "mid"), with noise."""
    out = []
    for name in ("plain", "flip", "PhiPi"):
        q = ko.rotation_from_euler(*EULERS[name])
        sim, _ = simulate(g.shape, np.ones(g.shape, bool), q, PCS["mid"], mp)
        noisy = sim + 0.4 * sim.std() * rng.standard_normal(sim.size)
        out.append(np.clip((noisy - noisy.min()) / (noisy.max() - noisy.min()) * 255, 0, 255).astype(np.uint8))
    return np.stack(out).reshape(N_PATTERNS, *g.shape)


@functools.lru_cache(maxsize=None)
def build_geometry(name):
    g = GEOMETRY[name]
    keep = keep_mask(g.shape, g.mask)
    k = int(keep.sum())
    assert k >= 8, (name, k)  # with a handful of pixels NCC is +-1 or noise: nothing to compare
    mp = master(g.master)
    for attempt in range(50):  # inputs whose prepared bits could depend on the summation order are replaced
        if g.mask == "circular-T":  # the patterns of 12x20-circular, transposed
            raw = np.ascontiguousarray(build_geometry("12x20-circular").raw.transpose(0, 2, 1))
        else:
            raw = experimental_patterns(g, keep, mp, np.random.default_rng([_seed(name), attempt]))
        if not any(order_complaints(p[keep], False) for p in raw):
            break
    else:
        raise AssertionError(f"{name}: no order-independent input in 50 draws")
    prepared = [prep64(p[keep], False) for p in raw]
    pat, sqn = np.stack([p[0] for p in prepared]), np.array([p[1] for p in prepared])
    evals = []
    for pc_name, pc in PCS.items():
        for eu_name, eu in EULERS.items():
            q = ko.rotation_from_euler(*eu)
            sim32, z = simulate(g.shape, keep, q, pc, mp)
            share = float(min((z >= 0).mean(), (z < 0).mean()))
            assert np.abs(z).min() > 1e-9, (name, pc_name, eu_name, np.abs(z).min())
            f, tol, ratio = zip(*(ncc_terms(sim32, pat[i], sqn[i]) for i in range(N_PATTERNS)))
            assert max(ratio) <= 1e6, (name, pc_name, eu_name, ratio)
            if (pc_name, eu_name) in TWO_HEMISPHERES:
                assert share >= 0.1, (name, pc_name, eu_name, share)
            evals.append(Evaluation(pc_name, eu_name, np.array(pc, float), np.array(eu, float), q, sim32, np.array(f),
                                    np.array(tol), share, float(np.abs(z).min()), max(ratio)))
    mask_out = None if g.mask == "none" else ~keep
    return BuiltGeometry(g, keep, mask_out, k, raw, pat, sqn, mp, tuple(evals))


def objective_batch(b, mode):
    """Everything kpdi_refine_objective takes for one mode: every evaluation of the geometry on the patterns
    PATTERN_INDEX.  Returns (pattern_index, x, fixed or None, expected, tolerance, labels)."""
    idx, x, fixed, want, tol, labels = [], [], [], [], [], []
    for e in b.evals:
        for i in PATTERN_INDEX:
            idx.append(i)
            if mode == ORI:
                x.append(e.eu), fixed.append(e.pc)
            elif mode == PC:
                x.append(e.pc), fixed.append(e.q)
            else:
                x.append(np.concatenate([e.eu, e.pc]))
            want.append(e.f[i]), tol.append(e.tol[i]), labels.append(f"{b.geom.name}/{e.pc_name}/{e.eu_name}/pattern{i}")
    return (np.array(idx, np.int32), np.array(x), np.array(fixed) if fixed else None, np.array(want), np.array(tol), labels)


# ---- the preparation matrix ---------------------------------------------------------------------------------------------
PREP_DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.int32, np.uint32, np.float32, np.float64, np.float16)
PREP_K = (8, 63, 64, 255, 256, 257, 1000)
# none of them square; the masked cases keep k pixels of a detector two rows and three columns larger
PREP_SHAPES = {8: (2, 4), 63: (7, 9), 64: (4, 16), 255: (15, 17), 256: (8, 32), 257: (1, 257), 1000: (25, 40)}
PrepCase = namedtuple("PrepCase", "name dtype rescale masked k shape recipe", defaults=(None,))
BuiltPrep = namedtuple("BuiltPrep", "case raw mask_out want_pat want_sqn")


def _prep_cases():
    out = []
    for dt in PREP_DTYPES:
        for rescale in (False, True):
            for masked in (False, True):
                for k in PREP_K:
                    r, c = PREP_SHAPES[k]
                    shape = (r + 2, c + 3) if masked else (r, c)
                    out.append(PrepCase(f"{np.dtype(dt).name}-{'rescale' if rescale else 'plain'}-"
                                        f"{'masked' if masked else 'whole'}-k{k}", np.dtype(dt), rescale, masked, k, shape))
    return out


# pattern 1 of three is the edge row; 257 of 7 x 37 pixels kept: two waves and one thread more
_EDGE_AT = {"first": 0, "wave1": 100, "last": 256}


def _edge_cases():
    out = []
    for dt, value in ((np.uint8, 7), (np.int16, -300), (np.uint32, 4000000001), (np.float32, 0.1), (np.float64, 0.1),
                      (np.float16, -2.5)):
        for rescale in (False, True):
            out.append(PrepCase(f"edge-constant-{np.dtype(dt).name}-{'rescale' if rescale else 'plain'}", np.dtype(dt), rescale,
                                True, 257, (7, 37), ("constant", value)))
    for dt in (np.float32, np.float64, np.float16):
        for what, value in (("nan", np.nan), ("inf", np.inf), ("neginf", -np.inf)):
            for where in _EDGE_AT:
                for rescale in (False, True):
                    out.append(PrepCase(f"edge-{what}-{where}-{np.dtype(dt).name}-{'rescale' if rescale else 'plain'}",
                                        np.dtype(dt), rescale, True, 257, (7, 37), (what, value, _EDGE_AT[where])))
    return out


PREP_CASES = _prep_cases()
EDGE_CASES = _edge_cases()
PREP = {c.name: c for c in PREP_CASES + EDGE_CASES}
assert len(PREP) == len(PREP_CASES) + len(EDGE_CASES)


def _raw_values(rng, dt, shape):
    """The whole range of an integer type (negative values, 32-bit values far above 2^24, which round on the cast);
    floats: multiples of 2^-16 in [-2, 2), for float64 with 2^-40 added so that the cast to float32 rounds."""
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    a = rng.integers(-2**17, 2**17, shape) / 2.0**16
    if dt == np.float64:
        a = a + rng.choice([-3.0, -1.0, 1.0, 3.0], shape) * 2.0**-40
    return a.astype(dt)


def _outside_values(dt, n):
    """What the pixels the mask drops hold: the extremes of the type, NaN and huge values for the floats."""
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return np.resize(np.array([info.max, info.min], dtype=dt), n)
    big = 6e4 if dt == np.float16 else 1e30
    return np.resize(np.array([np.nan, big, -big, np.inf], dtype=dt), n)


@functools.lru_cache(maxsize=None)
def build_prep(name):
    c = PREP[name]
    npix = c.shape[0] * c.shape[1]
    for attempt in range(50):
        rng = np.random.default_rng([_seed(name) % 2**31, len(name), attempt])
        raw = _raw_values(rng, c.dtype, (N_PATTERNS, npix))
        keep = np.ones(npix, bool)
        if c.masked:
            keep[rng.permutation(npix)[: npix - c.k]] = False
            raw[:, ~keep] = _outside_values(c.dtype, npix - c.k)
        assert keep.sum() == c.k
        if c.recipe is not None:
            kept = np.flatnonzero(keep)
            if c.recipe[0] == "constant":
                raw[1, kept] = np.array(c.recipe[1]).astype(c.dtype)
            else:
                raw[1, kept[c.recipe[2]]] = c.recipe[1]
        ordinary = [i for i in range(N_PATTERNS) if c.recipe is None or i != 1]
        if not any(order_complaints(raw[i, keep], c.rescale) for i in ordinary):
            break
    else:
        raise AssertionError(f"{name}: no order-independent input in 50 draws")
    want = [prep64(raw[i, keep], c.rescale) for i in range(N_PATTERNS)]
    return BuiltPrep(c, raw.reshape(N_PATTERNS, *c.shape), ~keep.reshape(c.shape) if c.masked else None,
                     np.stack([w[0] for w in want]), np.array([w[1] for w in want]))


def same_bits(got, want):
    """Bit for bit, any NaN standing for any other (the payload of a NaN is not part of the contract)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(u)[~nan], want.view(u)[~nan]))


# ---- the solve off the square -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_inputs():
    """12 synthetic 12 x 20 experiments for a complete refinement: circular mask, two hemispheres, starts up to 1 degree
    off.  Returns (uint8 patterns, keep, PC, true Euler angles, starts, master pattern)."""
    rng = np.random.default_rng(2024)
    shape, pc, mp, n = (12, 20), np.array(PCS["mid"]), master("odd"), 12
    keep = keep_mask(shape, "circular")
    eu = np.array(EULERS["plain"]) + rng.uniform(-0.15, 0.15, (n, 3))
    pats = []
    for e in eu:
        sim, z = simulate(shape, np.ones(shape, bool), ko.rotation_from_euler(*e), pc, mp)
        assert min((z >= 0).mean(), (z < 0).mean()) >= 0.1
        noisy = sim + 0.2 * sim.std() * rng.standard_normal(sim.size)
        pats.append(((noisy - noisy.min()) / (noisy.max() - noisy.min()) * 255).astype(np.uint8))
    eu0 = eu + np.deg2rad(rng.uniform(-1, 1, eu.shape))
    return np.stack(pats).reshape(n, *shape), keep, pc, eu, eu0, mp
