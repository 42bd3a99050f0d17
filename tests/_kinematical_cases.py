"""Case table of the kinematical master pattern tests: the reflector lists, the sizes, the reflector counts around the
LDS chunk of csrc/kinematical_plan.h, hemispheres and scalings.  Inputs are arithmetic on integers (identical on every
NumPy version); tests/golden/kinematical.npz stores them beside the reference's outputs (tools/gen_kinematical_golden.py)
and tests/test_host_kinematical.py checks that they regenerate bit for bit.

Shared by tools/gen_kinematical_golden.py, tests/test_host_kinematical.py and tests/test_gpu_kinematical.py."""

import itertools
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_HEADER = os.path.join(ROOT, "kikuchipy_amd", "csrc", "kinematical_plan.h")

A_NI = 3.5236       # lattice parameter, angstrom
WAVELENGTH = 0.08586  # electrons at 20 kV, angstrom
MIN_D = 0.5         # smallest interplanar spacing kept, angstrom
MAX_INDEX = 6


def plan_constant(name):
    text = open(PLAN_HEADER).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


CHUNK = plan_constant("KIN_CHUNK")
FORCED_CHUNK = 16   # KPDI_KINEMATICAL_CHUNK of the small reflector counts
CHUNK_LENGTHS = (1, 7, FORCED_CHUNK, 64, CHUNK)  # "the same result for every forced chunk length"


def ni_reflectors(max_index=MAX_INDEX, min_d=MIN_D):
    """(hkl (338, 3), theta, F complex) of fcc Ni: indices all odd or all even, |h|, |k|, |l| <= 6, d >= 0.5 angstrom,
    theta = arcsin(lambda |g| / 2a), |F| = 1 / (1 + |g|^2) with a phase that depends on hkl (|g| = |hkl|).  Other limits
    give the longer list of tools/bench_kinematical.py."""
    r = range(-max_index, max_index + 1)
    hkl = np.array([t for t in itertools.product(r, r, r)
                    if any(t) and len({abs(i) % 2 for i in t}) == 1], dtype=np.float64)
    g2 = np.sum(hkl**2, axis=1)
    hkl = hkl[A_NI / np.sqrt(g2) >= min_d]
    g2 = np.sum(hkl**2, axis=1)
    theta = np.arcsin(WAVELENGTH * np.sqrt(g2) / (2 * A_NI))
    modulus = 1.0 / (1.0 + g2)
    phase = 0.3 * (hkl[:, 0] + 2 * hkl[:, 1] + 3 * hkl[:, 2])
    return hkl, theta, modulus * (np.cos(phase) + 1j * np.sin(phase))


def unit_vectors(hkl):
    """`Vector3d(hkl).unit.data` for a cubic lattice."""
    return hkl / np.sqrt(np.sum(hkl**2, axis=-1))[:, np.newaxis]


def directions(half_size, pole):
    """Pixel directions (size * size, 3) of one hemisphere.  The two orix formulas the reference calls are restated here
    because orix is not installed: `InverseStereographicProjection(pole).xy2vector(x, y)` (orix/projections/
    stereographic.py) is (2x, 2y, -pole (1 - x^2 - y^2)) / (1 + x^2 + y^2); the upper hemisphere has pole -1."""
    size = 2 * half_size + 1
    arr = np.linspace(-1, 1, size)
    x, y = np.meshgrid(arr, arr)
    x, y = x.ravel(), y.ravel()
    denom = 1 + x**2 + y**2
    return np.column_stack([2 * x / denom, 2 * y / denom, -pole * (1 - x**2 - y**2) / denom])


def poles(hemisphere):
    return {"upper": [-1], "lower": [1], "both": [-1, 1]}[hemisphere]


def fma(a, b, c):
    """round(a * b + c) with one rounding (float(Fraction) rounds to nearest even)."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def dot_plain(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def dot_fma(u, v):
    return fma(u[2], v[2], fma(u[1], v[1], u[0] * v[0]))


PARALLEL_HALF_SIZE = 8


def parallel_reflector():
    """A pixel direction v of the half_size 8 upper grid whose squared length rounds to MORE than 1 as the reference adds
    it up and to at most 1 with contracted multiply-adds (the first such pixel in row-major order): as a reflector with
    theta = pi/2 (band: every angle in [0, pi/2]) the pixel itself gets nothing from the reference (acos(D > 1) is NaN)
    and the full intensity from a contracted dot product - no last bit of acos is involved."""
    for v in directions(PARALLEL_HALF_SIZE, -1):
        if dot_plain(v, v) > 1.0 >= dot_fma(v, v):
            return v.copy()
    raise AssertionError("no pixel of the half_size 8 grid separates the plain from the contracted dot product")


def handmade_reflectors():
    """(unit vectors, theta, F): one reflector along +z (D = 1 at the centre pixel), one in the equatorial plane (D exactly
    0 along the grid's central column), one with theta = 0 along (1, 1, 0) (D exactly 0 on the anti-diagonal, an empty
    band elsewhere), and `parallel_reflector()` with theta = pi/2."""
    s = np.sqrt(0.5)
    u = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [s, s, 0.0], parallel_reflector()])
    theta = np.array([0.02, 0.03, 0.0, np.pi / 2])
    f = np.array([1.0, 0.75 + 0j, 0.5j, 0.25], dtype=np.complex128)
    return u, theta, f


def intensity(f, scaling):
    """calculate_master_pattern's `match scaling` (simulations/kikuchi_pattern_simulator.py:169-181)."""
    if scaling == "linear":
        return abs(f)
    if scaling == "square":
        return abs(f * f.conjugate())
    assert scaling is None
    return np.ones(f.size)


def reflectors(which, m=None):
    """(unit vectors, theta, F) of a case's list: "ni" (its first `m`) or "handmade"."""
    if which == "handmade":
        return handmade_reflectors()
    hkl, theta, f = ni_reflectors()
    m = hkl.shape[0] if m is None else m
    return unit_vectors(hkl)[:m], theta[:m], f[:m]


def _case(name, which, m, half_size, hemisphere, scaling, chunk=None, golden=True):
    return {"name": name, "reflectors": which, "m": m, "half_size": half_size, "hemisphere": hemisphere, "scaling": scaling,
            "chunk": chunk, "golden": golden}


def cases():
    """Every case: `chunk` None is the library's own; `golden` False has no fixture entry (the restatement stands in)."""
    out = []
    for hs in (0, 1, 8, 20):      # one pixel; 3 x 3; 289 pixels: a ragged wave; 1681: several workgroups, a ragged last
        out.append(_case(f"ni_h{hs}_both", "ni", 338, hs, "both", "linear"))
    for hemisphere in ("upper", "lower"):
        out.append(_case(f"ni_h8_{hemisphere}", "ni", 338, 8, hemisphere, "linear"))
        out.append(_case(f"ni_h20_{hemisphere}", "ni", 338, 20, hemisphere, "linear", golden=False))
    out.append(_case("ni_h8_both_square", "ni", 338, 8, "both", "square"))
    out.append(_case("ni_h8_both_none", "ni", 338, 8, "both", None))
    for m in (1, FORCED_CHUNK - 1, FORCED_CHUNK, FORCED_CHUNK + 1):
        out.append(_case(f"ni_m{m}_c{FORCED_CHUNK}", "ni", m, 8, "upper", "linear", chunk=FORCED_CHUNK))
    for m in (CHUNK - 1, CHUNK, CHUNK + 1):
        out.append(_case(f"ni_m{m}", "ni", m, 8, "lower", "linear", golden=m == CHUNK + 1))
    for hs in (8, 20):
        out.append(_case(f"handmade_h{hs}_both", "handmade", 4, hs, "both", "linear"))
    out.append(_case("handmade_h8_upper_square", "handmade", 4, 8, "upper", "square"))
    return out


END_TO_END = _case("ni_h50_both", "ni", 338, 50, "both", "linear")  # its master pattern and as_lambert() are stored


def key(case):
    return "mp__" + case["name"]
