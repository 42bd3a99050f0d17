"""A float64 NumPy restatement of the reference's kinematical master pattern (`get_pattern`,
simulations/kikuchi_pattern_simulator.py:685-700, as `calculate_master_pattern` :162-199 calls it), vectorised over the
pixels: for every reflector in rising index the operations of the plain-Python loop, element by element, so a pixel's sum
has the loop's order and bits.  tests/test_host_kinematical.py pins it to tests/golden/kinematical.npz (the reference's own
function) bit for bit; the GPU tests use it where a case has no fixture entry.

The three `wrong` variants are what a test must be able to tell apart: "symmetric" (the band test on both sides of pi/2),
"no_half" (no half-intensity branch) and "fma" (D from contracted multiply-adds)."""

import numpy as np

import _kinematical_cases as cases

HALF_WIDTH = 1e-7


def dots(u, v, wrong=None):
    """D for reflector u (3,) and all directions v (n, 3)."""
    if wrong == "fma":
        return np.array([cases.dot_fma(u, vi) for vi in v])
    return (u[0] * v[:, 0] + u[1] * v[:, 1]) + u[2] * v[:, 2]


def get_pattern(intensity, xyz_hemi, xyz_reflector, theta_reflector, wrong=None, counts=None, screen=None):
    """The pattern (n,) of one hemisphere.  `counts`: a dict that receives the number of pairs per branch; `screen`: a
    margin in D - the number of pairs within it of cos(theta1) (those for which csrc/kinematical.hip evaluates acos) is
    counted as well."""
    theta2 = np.pi / 2
    theta1 = theta2 - theta_reflector
    pattern = np.zeros(xyz_hemi.shape[0], dtype=np.float64)
    tally = {"half": 0, "band": 0, "negative_in_mirror_band": 0, "d_ge_1": 0, "acos": 0, "pairs": 0}
    with np.errstate(invalid="ignore"):
        for i in range(xyz_reflector.shape[0]):
            d = dots(xyz_reflector[i], xyz_hemi, wrong)
            half = np.abs(d) <= HALF_WIDTH
            if wrong == "no_half":
                half = np.zeros_like(half)
            angle = np.arccos(d)
            if wrong == "symmetric":
                band = ~half & (angle <= theta2 + theta_reflector[i]) & (angle >= theta1[i])
            else:
                band = ~half & (angle <= theta2) & (angle >= theta1[i])
            pattern = np.where(half, pattern + 0.5 * intensity[i], np.where(band, pattern + intensity[i], pattern))
            if counts is not None:
                tally["half"] += int(half.sum())
                tally["band"] += int(band.sum())
                tally["negative_in_mirror_band"] += int((~half & (d < 0) & (np.abs(d) <= np.sin(theta_reflector[i]))).sum())
                tally["d_ge_1"] += int((d >= 1).sum())
                tally["pairs"] += d.size
                if screen is not None:
                    c = np.cos(theta1[i])
                    tally["acos"] += int(((d > HALF_WIDTH) & (d > c - screen) & (d < c + screen)).sum())
    if counts is not None:
        counts.update(tally)
    return pattern


def get_pattern_screened(intensity, xyz_hemi, xyz_reflector, theta_reflector, screen=1e-6):
    """The decisions of csrc/kinematical.hip in NumPy: acos only between the two thresholds of kin_screen
    (csrc/kinematical_plan.h), every other pair decided by D alone."""
    theta2 = np.pi / 2
    theta1 = theta2 - theta_reflector
    pattern = np.zeros(xyz_hemi.shape[0], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(xyz_reflector.shape[0]):
            if 0.0 <= theta1[i] <= 3.141592653589793:
                lo, hi = np.cos(theta1[i]) - screen, np.cos(theta1[i]) + screen
            else:
                lo, hi = -np.inf, np.inf
            d = dots(xyz_reflector[i], xyz_hemi)
            half = np.abs(d) <= HALF_WIDTH
            positive = ~half & (d > 0.0)
            inside = positive & (d <= lo)
            between = positive & ~inside & ~(d >= hi)
            angle = np.arccos(np.where(between, d, 0.0))
            inside |= between & (angle <= theta2) & (angle >= theta1[i])
            pattern = np.where(half, pattern + 0.5 * intensity[i], np.where(inside, pattern + intensity[i], pattern))
    return pattern


def near_threshold(xyz_hemi, xyz_reflector, theta_reflector, margin=1e-12):
    """Pixels (n,) bool that the GPU comparison may leave out: for some reflector whose pair evaluates acos (|D| > 1e-7)
    |acos(D) - (pi/2 - theta)| or |acos(D) - pi/2| is below `margin`, or for any reflector ||D| - 1e-7| is.  (A pair with
    |D| <= 1e-7 is decided by D alone: D exactly 0, where acos(D) is pi/2, is no reason to leave a pixel out.)"""
    theta2 = np.pi / 2
    out = np.zeros(xyz_hemi.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for i in range(xyz_reflector.shape[0]):
            d = dots(xyz_reflector[i], xyz_hemi)
            angle = np.arccos(d)
            near = (np.abs(angle - (theta2 - theta_reflector[i])) < margin) | (np.abs(angle - theta2) < margin)
            out |= near & (np.abs(d) > HALF_WIDTH)
            out |= np.abs(np.abs(d) - HALF_WIDTH) < margin
    return out


def master_pattern(case, wrong=None, counts=None, screen=None):
    """calculate_master_pattern's data for a case of tests/_kinematical_cases.py: (size, size) or (2, size, size)."""
    u, theta, f = cases.reflectors(case["reflectors"], case["m"])
    inten = cases.intensity(f, case["scaling"])
    size = 2 * case["half_size"] + 1
    total = {}
    out = []
    for pole in cases.poles(case["hemisphere"]):
        c = {} if counts is not None else None
        out.append(get_pattern(inten, cases.directions(case["half_size"], pole), u, theta, wrong, c, screen))
        if c is not None:
            for k, v in c.items():
                total[k] = total.get(k, 0) + v
    if counts is not None:
        counts.update(total)
    out = np.array(out).reshape(-1, size, size)  # (the reference squeezes; a 1 x 1 pattern keeps its two axes here)
    return out if case["hemisphere"] == "both" else out[0]


def left_out(case):
    """`near_threshold` in the shape of `master_pattern(case)`."""
    u, theta, _ = cases.reflectors(case["reflectors"], case["m"])
    out = [near_threshold(cases.directions(case["half_size"], pole), u, theta) for pole in cases.poles(case["hemisphere"])]
    size = 2 * case["half_size"] + 1
    out = np.array(out).reshape(-1, size, size)
    return out if case["hemisphere"] == "both" else out[0]
