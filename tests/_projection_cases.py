"""Probes of the master-pattern projection (csrc/projection.h, csrc/project.hip) and a plain restatement of what it
computes in `np.longdouble`, shared by tests/test_host_projection.py (CPU) and tests/test_gpu_projection_probes.py.

How the kernel is read out: with the identity rotation, `set_direction_cosines(probes)`, float64 output and no
rescale, output pixel c is `project_pixel(probes[c])`.  On a master pattern `upper[r][c] = r` bilinear interpolation
returns the Lambert Y of the probe in master-pattern pixels (row coordinate), on `upper[r][c] = c` the Lambert X
(column coordinate), and `lower = upper + 1000` makes the value name the hemisphere: the kernel becomes a float64
evaluator of `_vector2lambert` + `_get_lambert_interpolation_parameters` (signals/util/_master_pattern.py:530-678).

`project_ld` states those formulas (and rotate_vector, _utils/numba.py:59-81, and the bilinear sum, :682-708) with
64-bit mantissas and the mathematical constants, and keeps the reference's conventions: `abs_z == 1` is (0, 0),
`|y| <= |x|` is the x-dominant branch, `z >= 0` reads the upper hemisphere, a neighbour beyond the last row / column
is the row / column itself.

Tolerance of a float64 kernel output: `4 * FLOOR[class][npx] + 8 * ulp(|value|)`.  FLOOR is what an honest float64
evaluation of the reference's formulas with libm (oracle.kpdi_oracle.project_patterns) loses against `project_ld` on
the ramp master patterns, in master-pattern pixels, per probe class (near-pole probes are ill-conditioned in float64:
1 - |z| cancels) and per master-pattern size (the coordinates scale with it, so one figure for every size would be
400 times too wide at npx = 2).  The factor 4: projection.h claims its helpers agree with libm "to the last bit or
two", that is up to twice libm's error per helper, through a chain of two such helpers (normalise / square root, then
arctan).  8 ulp: the at most seven roundings of the bilinear sum itself.  Neither number is fitted to kernel output.
The `generic` floor holds down to the pole distance at which it was measured (`generic_pole_distance`).  The few
rotated directions of the varying-PC and path-boundary tests that come nearer a pole (`near_pole`) have floors of
their own, measured in the same way at those very directions: FLOOR["varying_pc_near_pole"],
FLOOR["path_boundary_near_pole"].
"""

import os
import sys

import numpy as np

LD = np.longdouble
HAVE_LD = np.finfo(LD).eps < 2e-19  # x87 extended or better; the tests skip otherwise
PI = 4 * np.arctan(LD(1))
SQRT_PI = np.sqrt(PI)
SQRT_HALF_PI = np.sqrt(PI / 2)
ATAN_SEAM = 0.41421356237309503  # tan(pi / 8): where atan_ratio switches to pi/4 + atan((a - b) / (a + b))
NPX = (2, 11, 12, 401)
IDENTITY = np.array([[1.0, 0.0, 0.0, 0.0]])


# ------------------------------------------------------------------ the restatement
def rotate_ld(q, p):
    """rotate_vector: passive rotation of (n, 3) vectors by (a, b, c, d), which is NOT normalised first."""
    a, b, c, d = (LD(t) for t in q)
    x, y, z = (np.asarray(p[:, k], dtype=LD) for k in range(3))
    aa, bb, cc, dd = a * a, b * b, c * c, d * d
    ac, ab, ad, bc, bd, cd = a * c, a * b, a * d, b * c, b * d, c * d
    return np.stack([(aa + bb - cc - dd) * x + 2 * ((ac + bd) * z + (bc - ad) * y),
                     (aa - bb + cc - dd) * y + 2 * ((ad + bc) * x + (cd - ab) * z),
                     (aa - bb - cc + dd) * z + 2 * ((ab + cd) * y + (bd - ac) * x)], axis=1)


def lambert_ld(v, arctan=np.arctan):
    """_vector2lambert: square Lambert (X, Y) in [-sqrt(pi/2), sqrt(pi/2)] of (n, 3) long-double vectors."""
    w = v / np.sqrt(np.sum(v * v, axis=1))[:, None]
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    abs_z = np.abs(z)
    sqrt_z = np.sqrt(2 * (1 - abs_z))
    pole = abs_z == 1
    xdom = (np.abs(y) <= np.abs(x)) & ~pole
    ydom = ~xdom & ~pole
    X, Y = np.zeros(len(v), LD), np.zeros(len(v), LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        sx, sy = np.sign(x), np.sign(y)
        X[xdom] = (sx * sqrt_z * (SQRT_PI / 2))[xdom]
        Y[xdom] = (sx * sqrt_z * (2 / SQRT_PI) * arctan(y / x))[xdom]
        X[ydom] = (sy * sqrt_z * (2 / SQRT_PI) * arctan(x / y))[ydom]
        Y[ydom] = (sy * sqrt_z * (SQRT_PI / 2))[ydom]
    return X, Y


def project_ld(rotations, probes, upper, lower=None, *, arctan=np.arctan, zero_is_upper=True, swap_rows_columns=False,
               edge="repeat"):
    """(n rotations, n probes) long-double intensities.  The keyword arguments exist for the mutation checks of
    tests/test_host_projection.py only; their defaults are the reference."""
    upper = np.asarray(upper)
    lower = upper if lower is None else np.asarray(lower)
    npy, npx = upper.shape
    scale = LD(npx - 1) / 2
    mps = np.stack([upper, lower]).astype(LD)
    out = np.empty((len(rotations), len(probes)), LD)
    for n, q in enumerate(np.asarray(rotations, dtype=np.float64).reshape(-1, 4)):
        v = rotate_ld(q, np.asarray(probes, dtype=np.float64))
        X, Y = lambert_ld(v, arctan)
        i, j = scale * Y / SQRT_HALF_PI, scale * X / SQRT_HALF_PI  # row from Lambert Y, column from Lambert X
        nii, nij = np.trunc(i + scale).astype(np.int64), np.trunc(j + scale).astype(np.int64)
        niip, nijp = nii + 1, nij + 1
        if edge == "repeat":
            niip, nijp = np.where(niip >= npx, nii, niip), np.where(nijp >= npy, nij, nijp)
        else:  # mutant: wrap around
            niip, nijp = niip % npx, nijp % npy
        nii, nij = np.where(nii < 0, niip, nii), np.where(nij < 0, nijp, nij)
        di, dj = i - nii + scale, j - nij + scale
        dim, djm = 1 - di, 1 - dj
        h = np.where(v[:, 2] >= 0 if zero_is_upper else v[:, 2] > 0, 0, 1)
        if swap_rows_columns:  # mutant
            nii, nij, niip, nijp = nij, nii, nijp, niip
        out[n] = (mps[h, nii, nij] * dim * djm + mps[h, niip, nij] * di * djm
                  + mps[h, nii, nijp] * dim * dj + mps[h, niip, nijp] * di * dj)
    return out


def rescale_ld(patterns, out_min, out_max):
    """_rescale_with_min_max (pattern/_pattern.py:97-111) of every row over its own minimum and maximum."""
    lo, hi = patterns.min(axis=1, keepdims=True), patterns.max(axis=1, keepdims=True)
    return (patterns - lo) / (hi - lo) * (LD(out_max) - LD(out_min)) + LD(out_min)


def inverse_lambert_ld(X, Y, hemisphere):
    """Unit vectors (long double) whose square Lambert coordinates are (X, Y); hemisphere +1: z >= 0, -1: z <= 0.
    From the forward formulas: x-dominant |z| = 1 - 2 X^2 / pi and atan(y / x) = pi Y / (4 X)."""
    X, Y = np.atleast_1d(np.asarray(X, LD)), np.atleast_1d(np.asarray(Y, LD))
    xdom = np.abs(Y) <= np.abs(X)
    a, b = np.where(xdom, X, Y), np.where(xdom, Y, X)  # along the dominant axis, across it
    m = np.minimum(2 * a * a / PI, LD(1))  # 1 - |z|
    rho = np.sqrt(m * (2 - m))  # sqrt(1 - z^2) without cancellation at the poles
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(a == 0, LD(0), PI * b / (4 * a))
    major, minor = np.sign(a) * rho * np.cos(phi), np.sign(a) * rho * np.sin(phi)
    return np.stack([np.where(xdom, major, minor), np.where(xdom, minor, major), hemisphere * (1 - m)], axis=1)


# ------------------------------------------------------------------ master patterns
def masters(kind, npx, offset=1000):
    """(upper, lower) float32: 'row' upper[r][c] = r, 'col' upper[r][c] = c, lower = upper + offset (exact in
    float32); 'random' two independent uniform hemispheres; 'moat' 1 everywhere but 2^100 in the first row and the
    first column of both hemispheres: a read that wraps around from the last row / column shows at any non-zero
    weight (on the equator that weight is rounding noise, and tests/test_host_projection.py asserts that it shows)."""
    if kind == "moat":
        up = np.ones((npx, npx), np.float32)
        up[0], up[:, 0] = 2.0 ** 100, 2.0 ** 100
        return up, up.copy()
    if kind == "random":
        rng = np.random.default_rng(1000 + npx)
        return rng.random((npx, npx)).astype(np.float32), rng.random((npx, npx)).astype(np.float32)
    r, c = np.meshgrid(np.arange(npx), np.arange(npx), indexing="ij")
    up = (r if kind == "row" else c).astype(np.float32)
    return up, up + np.float32(offset)


# ------------------------------------------------------------------ probe classes: (n, 3) float64 and the class name
def _signs2():
    return [(sx, sy) for sx in (1.0, -1.0) for sy in (1.0, -1.0)]


def poles():
    p = [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    for e in (10, 20, 26, 27, 30, 40, 200):
        t = 2.0 ** -e
        for z in (1.0, -1.0):
            p += [(t, 0.0, z), (0.0, t, z), (t, -t, z)]
    return np.array(p), "poles"


def equator():
    az = np.concatenate([np.arange(8) * (np.pi / 4), np.random.default_rng(11).uniform(0, 2 * np.pi, 16)])
    xy = np.stack([np.cos(az), np.sin(az)], axis=1)
    xy[:8] = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]  # axes and diagonals exactly
    p = [(x, y, z) for x, y in xy for z in (0.0, -0.0, 2.0 ** -60, -(2.0 ** -60))]
    return np.array(p), "equator"


def far_edge(npx):
    """The equator probes whose bilinear footprint stays clear of the first row and column (coordinates >= 1.5): on
    the 'moat' master pattern they read exactly 1, along the last row / column through the edge rule."""
    p = equator()[0]
    scale = LD(npx - 1) / 2
    X, Y = lambert_ld(np.asarray(p, dtype=LD))
    return p[(scale * Y / SQRT_HALF_PI + scale >= 1.5) & (scale * X / SQRT_HALF_PI + scale >= 1.5)], "equator"


def diagonals():
    p = []
    for z in (0.1, -0.1, 0.5, -0.5, 0.9, -0.9):
        for a in (np.sqrt((1 - z * z) / 2), 1.0):  # unit length, and not
            p += [(sx * a, sy * a, z) for sx, sy in _signs2()]
    return np.array(p), "diagonals"


def axes_and_octants():
    p = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0)]
    g = np.array([0.37, 0.61, 0.7])
    g /= np.linalg.norm(g)
    for f in (1.0, 1e-3, 1e3):
        p += [tuple(f * g * (sx, sy, sz)) for sx, sy in _signs2() for sz in (1.0, -1.0)]
    return np.array(p), "axes_and_octants"


def atan_seam():
    minors = [ATAN_SEAM]
    for _ in range(4):
        minors = [np.nextafter(minors[0], 0.0)] + minors + [np.nextafter(minors[-1], 1.0)]
    p = []
    for m in minors:
        for sx, sy in _signs2():
            p += [(sx, sy * m, 0.5), (sx * m, sy, 0.5)]
    return np.array(p), "atan_seam"


def atan_sweep():
    ratios = np.concatenate([np.arange(2049) / 2048.0, [2.0 ** -30, 2.0 ** -100, 1e-300]])
    one, half = np.ones_like(ratios), np.full_like(ratios, 0.5)
    return np.concatenate([np.stack([one, ratios, half], axis=1), np.stack([ratios, one, half], axis=1)]), "atan_sweep"


def lattice_nodes(npx, every_node=False):
    """(rows, columns, hemispheres) of the `lattice` class: every node up to npx = 12, nine rows x nine columns (first,
    last, centre and their neighbours) above, where only `every_node` gives them all (320 002 probes: for the GPU
    alone, which is to return mp[r][c]).  A node on the outer edge is on the equator (z = 0), which reads upper, so
    the lower hemisphere has the inner nodes only."""
    k = np.arange(npx) if npx <= 12 or every_node else np.array([0, 1, 2, npx // 2 - 1, npx // 2, npx // 2 + 1, npx - 3, npx - 2, npx - 1])
    r, c = (t.ravel() for t in np.meshgrid(k, k, indexing="ij"))
    inner = (r > 0) & (r < npx - 1) & (c > 0) & (c < npx - 1)
    return (np.concatenate([r, r[inner]]), np.concatenate([c, c[inner]]),
            np.concatenate([np.ones(r.size, int), -np.ones(inner.sum(), int)]))


def lattice(npx, every_node=False):
    r, c, h = lattice_nodes(npx, every_node)
    scale = LD(npx - 1) / 2
    v = inverse_lambert_ld((c - scale) / scale * SQRT_HALF_PI, (r - scale) / scale * SQRT_HALF_PI, h)
    return v.astype(np.float64), "lattice"


def generic(n=4096, seed=2024):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None], "generic"


def generic_pole_distance():
    """The smallest 1 - |z| among the generic probes: the `generic` floor was measured no closer to a pole than this
    (the error of a float64 evaluation grows like 1 / (1 - |z|) there)."""
    p = generic()[0].astype(LD)
    return float((1 - np.abs(p[:, 2]) / np.sqrt(np.sum(p * p, axis=1))).min())


def near_pole(rotations, probes):
    """(n rotations, n probes) mask of the rotated directions nearer a pole than that."""
    out = []
    for q in rotations:
        v = rotate_ld(q, probes)
        out.append(1 - np.abs(v[:, 2]) / np.sqrt(np.sum(v * v, axis=1)) < generic_pole_distance())
    return np.array(out)


FIXED_CLASSES = (poles, equator, diagonals, axes_and_octants, atan_seam, atan_sweep, generic)
CLASS_NAMES = tuple(f.__name__ for f in FIXED_CLASSES) + ("lattice",)


def probes_of(name, npx):
    return lattice(npx)[0] if name == "lattice" else globals()[name]()[0]


def readout_cases(npx):
    """(master kind, class name, probes, upper, lower) of the probe readout at one master-pattern size."""
    for kind in ("row", "col", "random"):
        up, lo = masters(kind, npx)
        for name in CLASS_NAMES:
            yield kind, name, probes_of(name, npx), up, lo
    if npx > 2:  # at npx = 2 every footprint touches the first row or column
        yield ("moat", "equator", far_edge(npx)[0]) + masters("moat", npx)


def rotation_set():
    """The eight quaternions of the rotation test.  The reference normalises none of them."""
    q = np.random.default_rng(8).standard_normal((3, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    h = np.sqrt(0.5)
    neg = np.array([-0.3, 0.5, -0.1, 0.8])
    return np.array([q[0], q[1], neg / np.linalg.norm(neg),  # two random unit ones, one with a < 0
                     [0.0, 1.0, 0.0, 0.0],                   # half turn about x: upper <-> lower
                     [h, 0.0, 0.0, h],                       # 90 degrees about z
                     0.5 * q[2], 2.0 * q[2],                 # not of unit length
                     [1.0, 0.0, 0.0, 0.0]])


def near_equator(rotations, probes):
    """(n rotations, n probes) mask: long-double |vz| below 1e-12 of the vector's length, where a float64 evaluation
    may name the other hemisphere."""
    out = []
    for q in rotations:
        v = rotate_ld(q, probes)
        out.append(np.abs(v[:, 2]) < 1e-12 * np.sqrt(np.sum(v * v, axis=1)))
    return np.array(out)


def path_boundary_case():
    """(probes (5000, 3), three quaternions, mask (3, 5000) of the rotated probes nearer a pole than any generic probe)
    of the path-boundary test, whose pixel counts are prefixes of the probes."""
    p, q = generic(5000, seed=77)[0], rotation_set()[:3]
    return p, q, near_pole(q, p)


def varying_pc_case(shape):
    """(quaternions, PCs, detector -> sample matrix, the oracle's direction cosines per PC, mask (3, npix) of the
    pixels that look closer to a pole than any generic probe) of the varying-PC test on one detector shape."""
    from oracle import kpdi_oracle as ko

    pcs = np.array([0.45, 0.6, 0.55]) + np.random.default_rng(shape[0]).uniform(-0.05, 0.05, (3, 3))
    q = rotation_set()[:3]
    om = ko.sample_to_detector_matrix(70.0, 10.0, 2.0, 1.0).T
    dcs = [ko.direction_cosines_fixed_pc(ko.gnomonic_bounds(shape, c), c[2], shape[0], shape[1], om) for c in pcs]
    return q, pcs, om, dcs, np.array([near_pole(q[i:i + 1], dcs[i])[0] for i in range(3)])


# ------------------------------------------------------------------ integer outputs: 64 rotations x generic probes
INT_NPIX = (600, 4100)  # register-resident, and the recompute path
INT_NPX = 101
_cache = {}


def integer_case():
    """(quaternions (64, 4), probes (4100, 3), random float32 master pattern, long-double patterns (64, 4100)); a
    prefix of the probes is a prefix of every pattern.  Computed once."""
    if "int" not in _cache:
        q = np.random.default_rng(64).standard_normal((64, 4))
        q /= np.linalg.norm(q, axis=1)[:, None]
        p = generic(INT_NPIX[-1], seed=600)[0]
        up, lo = masters("random", INT_NPX)
        _cache["int"] = (q, p, up, lo, project_ld(q, p, up, lo))
    return _cache["int"]


def integer_case_plain():
    """The same without rescale: a master pattern with values in [0, 250] and its long-double patterns."""
    if "plain" not in _cache:
        q, p, up, lo, _ = integer_case()
        up, lo = (up * 250).astype(np.float32), (lo * 250).astype(np.float32)
        _cache["plain"] = (up, lo, project_ld(q, p, up, lo))
    return _cache["plain"]


# ------------------------------------------------------------------ the yardstick
# max |oracle.kpdi_oracle.project_patterns (float64, libm) - project_ld| over the row and column ramps (both
# hemispheres the plain ramp, so that the figure is the coordinate's error and not the rounding of 1000 + r), identity
# rotation, in master-pattern pixels, rounded up to two digits.  Produced by: python tests/_projection_cases.py
FLOOR = {
    "poles": {2: 5.4e-9, 11: 5.4e-8, 12: 5.9e-8, 401: 2.2e-6},
    "equator": {2: 1.8e-16, 11: 2.2e-15, 12: 2.2e-15, 401: 4.7e-14},
    "diagonals": {2: 1.2e-16, 11: 2.0e-15, 12: 1.8e-15, 401: 7.5e-14},
    "axes_and_octants": {2: 1.6e-16, 11: 1.1e-15, 12: 1.2e-15, 401: 4.1e-14},
    "atan_seam": {2: 1.2e-16, 11: 2.2e-15, 12: 2.0e-15, 401: 6.6e-14},
    "atan_sweep": {2: 2.3e-16, 11: 3.9e-15, 12: 3.3e-15, 401: 1.5e-13},
    "generic": {2: 9.6e-16, 11: 9.9e-15, 12: 1.2e-14, 401: 4.2e-13},
    "lattice": {2: 1.2e-16, 11: 9.0e-16, 12: 1.9e-15, 401: 1.2e-12},
    # the same under the tests' own rotations, at the directions nearer a pole than any generic probe
    "varying_pc_near_pole": {401: 1.6e-12},
    "path_boundary_near_pole": {401: 4.0e-12},
}
NEAR_POLE_CASES = ("varying_pc_near_pole", "path_boundary_near_pole")


def measure_floor(name, npx):
    from oracle import kpdi_oracle as ko

    p = probes_of(name, npx)
    worst = 0.0
    for kind in ("row", "col"):
        up, lo = masters(kind, npx, offset=0)  # the coordinate alone: roundings at 1000 + r belong to the ulp term
        got = ko.project_patterns(IDENTITY, p, up, lo, dtype_out=np.float64)
        worst = max(worst, float(np.abs(got - project_ld(IDENTITY, p, up, lo)).max()))
    return worst


def near_pole_case(name):
    """(quaternions, probes per quaternion, mask of the directions nearer a pole than any generic probe)."""
    if name == "varying_pc_near_pole":
        q, _, _, probes, polar = varying_pc_case((70, 90))
        return q, probes, polar
    p, q, polar = path_boundary_case()
    return q, [p] * len(q), polar


def measure_near_pole(name, npx=401):
    """(float64 + libm error at the near-pole directions of a case, and at all its other directions)."""
    from oracle import kpdi_oracle as ko

    q, probes, polar = near_pole_case(name)
    worst_polar = worst_rest = 0.0
    for kind in ("row", "col"):
        up, lo = masters(kind, npx, offset=0)
        for i in range(len(q)):
            err = np.abs(ko.project_patterns(q[i:i + 1], probes[i], up, lo, dtype_out=np.float64)[0]
                         - project_ld(q[i:i + 1], probes[i], up, lo)[0]).astype(np.float64)
            worst_rest = max(worst_rest, float(err[~polar[i]].max()))
            worst_polar = max([worst_polar] + err[polar[i]].tolist())
    return worst_polar, worst_rest


def tolerance(name, npx, want):
    return 4 * FLOOR[name][npx] + 8 * np.spacing(np.abs(np.asarray(want, dtype=np.float64)))


def check_values(got, want, name, npx, label=""):
    """The comparison of every float64 test: no NaN, |got - want| <= tolerance.  Returns the largest error in units
    of its tolerance."""
    got = np.asarray(got)
    assert got.shape == np.shape(want), (got.shape, np.shape(want))
    assert not np.isnan(got).any(), f"{label} {name} npx={npx}: NaN in the output"
    ratio = (np.abs(got.astype(LD) - want) / tolerance(name, npx, want)).astype(np.float64)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{label} {name} npx={npx}: worst error / tolerance = {worst:.3g}")
    assert worst <= 1.0, f"{label} {name} npx={npx}: error {worst:.3g} x tolerance at pixel {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


def check_integer_patterns(got, want, out_min=None, out_max=None, label=""):
    """Integer outputs against the long-double values `want` (already rescaled, if the kernel rescaled).  With
    out_min / out_max: every pattern's minimum is exactly out_min and its maximum exactly out_max, at the reference's
    darkest and brightest pixel, and those two pixels leave the comparison.  Every other pixel is the truncation of `want`, except where `want` lies
    within 1e-9 of an integer; those exceptions are at most 0.1 % of the pixels.  Returns the exceptions' share."""
    got = np.asarray(got)
    assert got.shape == want.shape
    keep = np.ones(want.shape, bool)
    if out_min is not None:
        mins, maxs = got.min(axis=1), got.max(axis=1)
        assert (mins == out_min).all(), f"{label}: pattern minimum {mins[mins != out_min][:4]} != {out_min} in {np.sum(mins != out_min)} patterns"
        assert (maxs == out_max).all(), f"{label}: pattern maximum {maxs[maxs != out_max][:4]} != {out_max} in {np.sum(maxs != out_max)} patterns"
        rows = np.arange(len(want))
        darkest, brightest = want.argmin(axis=1), want.argmax(axis=1)
        assert (got[rows, darkest] == out_min).all() and (got[rows, brightest] == out_max).all(), f"{label}: out_min / out_max not at the reference's darkest / brightest pixel"
        keep[rows, darkest] = False
        keep[rows, brightest] = False
    near = np.abs(want - np.rint(want)) <= 1e-9
    bad = keep & ~near & (got.astype(np.int64) != np.trunc(want).astype(np.int64))
    assert not bad.any(), f"{label}: {bad.sum()} pixels are not the truncated reference value, first at {np.argwhere(bad)[0]}"
    share = float((keep & near).mean())
    print(f"{label}: {int((keep & near).sum())} pixels within 1e-9 of an integer left out")
    assert share <= 1e-3, f"{label}: {share:.2e} of the pixels left out"
    return share


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("FLOOR = {")
    for cls in CLASS_NAMES:
        cells = []
        for n in NPX:
            m, e = f"{measure_floor(cls, n):.1e}".split("e")  # two digits, rounded up
            cells.append(f"{n}: {float(m) + 0.1:.1f}e{int(e)}" if float(m) else f"{n}: 0.0")
        print(f'    "{cls}": {{{", ".join(cells)}}},')
    for cls in NEAR_POLE_CASES:
        m, e = f"{measure_near_pole(cls)[0]:.1e}".split("e")
        print(f'    "{cls}": {{401: {float(m) + 0.1:.1f}e{int(e)}}},')
    print("}")
