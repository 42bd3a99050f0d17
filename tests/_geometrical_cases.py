"""Case table of the geometrical simulation tests (KikuchiPatternSimulator.on_detector) and a NumPy float64 restatement
of the reference: the matrix chain of simulations/kikuchi_pattern_simulator.py:254-353, KikuchiPatternLine and
KikuchiPatternZoneAxis of simulations/_kikuchi_pattern_features.py, and the two detector-coordinate setters of
simulations/_kikuchi_pattern_simulation.py:468-534, with the reference's expressions (arccos / tan / arctan2 / cos / sin).
orix is not installed: its `Rotation.to_matrix` (orix/quaternion/_conversions.py, qu2om), `Vector3d.polar` / `.azimuth`
(orix/vector/vector3d.py) and `Miller.round().unique()` are restated, the last as "divide by the gcd, unique,
lexicographic order", which is this package's documented order.

Inputs are seeded or arithmetic on integers; tests/golden/geometrical.npz stores them beside the outputs of the
reference's own classes (tools/gen_geometrical_golden.py).

Shared by tools/gen_geometrical_golden.py, tests/test_host_geometrical.py and tests/test_gpu_geometrical.py."""

import itertools
import math
import os

import numpy as np

from kikuchipy_amd.detectors import EBSDDetector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_HEADER = os.path.join(ROOT, "kikuchipy_amd", "csrc", "geometrical_plan.h")
GOLDEN_KIN = os.path.join(ROOT, "tests", "golden", "kinematical.npz")

FORCED_CHUNK = 16  # KPDI_GEOMETRICAL_CHUNK of the chunk-independence test (the library's own: 64 points)
LEFT_OUT_CAP = 0.005


# ---- inputs ---------------------------------------------------------------------------------------------------------
def ni_hkl():
    """The Ni list of the kinematical fixtures (338 reflectors, integers)."""
    return np.load(GOLDEN_KIN)["in__ni__hkl"]


def family_111():
    hkl = ni_hkl()
    return hkl[np.all(np.abs(hkl) == 1, axis=1)]


def handmade_hkl(max_index=4, length=257):
    """Every hkl with indices up to `max_index` but [000], in the order of itertools.product, cut to `length`."""
    r = range(-max_index, max_index + 1)
    return np.array([t for t in itertools.product(r, r, r) if any(t)], dtype=np.float64)[:length]


def random_rotations(seed, shape, spread=None):
    """Unit quaternions of `shape` + (4,); `spread`: all within that much of one random rotation."""
    rng = np.random.default_rng(seed)
    if spread is None:
        q = rng.standard_normal(tuple(shape) + (4,))
    else:
        q = rng.standard_normal(4) + spread * rng.standard_normal(tuple(shape) + (4,))
    return q / np.sqrt(np.sum(q**2, axis=-1))[..., np.newaxis]


def random_pcs(seed, shape):
    rng = np.random.default_rng(seed)
    return np.array([0.42, 0.22, 0.5]) + 0.02 * (rng.random(tuple(shape) + (3,)) - 0.5)


TRICLINIC = np.array([[0.31, 0.02, -0.01], [-0.05, 0.22, 0.03], [0.04, -0.06, 0.17]])  # rows a*, b*, c*: no right angle
THIN = np.diag([5e-6, 1.0, 1.0])  # with an untilted detector and the identity rotation, z on the detector is 5e-6 h


def _case(name, hkl, nav, *, basis=None, pcs=None, seed=0, spread=None, det=None, rotations=None, golden=True, exact=False):
    det = dict(shape=(60, 60), sample_tilt=70.0, tilt=0.0) if det is None else det
    rot = random_rotations(seed, nav, spread) if rotations is None else rotations
    pc = np.array([0.4198, 0.2136, 0.5015]) if pcs is None else pcs
    return {"name": name, "hkl": np.asarray(hkl, dtype=np.float64), "basis": np.eye(3) if basis is None else basis,
            "rotations": rot, "pc": pc, "det": det, "golden": golden, "exact": exact}


def cases():
    """`golden` False has no fixture entry (the restatement stands in); `exact`: the reflectors with z = 0 and
    z = -5e-6 at the first point are decided by exact comparisons, so the |z| rule leaves nothing out there."""
    ni = ni_hkl()
    identity = np.array([1.0, 0.0, 0.0, 0.0])
    two = np.stack([identity, random_rotations(8, ())])
    return [
        _case("one_point_one_reflector", [[1, 1, 1]], (1,), seed=8),
        _case("one_point_111_family", family_111(), (1,), seed=2),
        _case("map3x3_nine_pcs", ni[::6], (3, 3), pcs=random_pcs(11, (3, 3)), seed=3, spread=0.2),
        _case("map3x3_one_pc", ni[::6], (3, 3), seed=4, spread=0.2),
        _case("line5", ni[3::13], (5,), pcs=random_pcs(12, (5,)), seed=6),
        _case("points65_reflectors257", handmade_hkl(), (65,), seed=7, spread=0.05, golden=False),
        _case("triclinic_2x2", handmade_hkl(2, 124)[::3], (2, 2), basis=TRICLINIC, seed=9, det=dict(shape=(48, 64), sample_tilt=70.0, tilt=5.0)),
        _case("handmade_z0", [[0, 1, 0], [-1, 1, 0], [1, 0, 0], [0, 0, 1], [1, 1, 1], [2, -1, 1]], (2,), basis=THIN, rotations=two,
              det=dict(shape=(60, 60), sample_tilt=0.0, tilt=0.0), pcs=np.array([0.5, 0.5, 0.5]), exact=True),
    ]


def detector(case):
    return EBSDDetector(pc=case["pc"], **case["det"])


# ---- the restatement ------------------------------------------------------------------------------------------------
def to_matrix(q):
    """orix/quaternion/_conversions.py, qu2om (what Rotation.to_matrix evaluates), for (n, 4) unit quaternions."""
    a, b, c, d = (q[:, i] for i in range(4))
    qq = a**2 - (b**2 + c**2 + d**2)
    om = np.empty((q.shape[0], 3, 3))
    om[:, 0, 0] = qq + 2 * b**2
    om[:, 1, 1] = qq + 2 * c**2
    om[:, 2, 2] = qq + 2 * d**2
    om[:, 0, 1] = 2 * (b * c - a * d)
    om[:, 1, 0] = 2 * (c * b + a * d)
    om[:, 1, 2] = 2 * (c * d - a * b)
    om[:, 2, 1] = 2 * (d * c + a * b)
    om[:, 2, 0] = 2 * (d * b - a * c)
    om[:, 0, 2] = 2 * (b * d + a * c)
    return om


def zone_axes_brute_force(hkl):
    """Reduced cross products of all ordered pairs, one triplet at a time with math.gcd; a sorted set."""
    found = set()
    rows = [tuple(int(v) for v in row) for row in hkl]
    for (h1, k1, l1), (h2, k2, l2) in itertools.product(rows, rows):
        u, v, w = k1 * l2 - l1 * k2, l1 * h2 - h1 * l2, h1 * k2 - k1 * h2
        g = math.gcd(math.gcd(abs(u), abs(v)), abs(w))
        if g:
            found.add((u // g, v // g, w // g))
    return np.array(sorted(found), dtype=np.float64).reshape(-1, 3)


def widened_ranges(det):
    """x_range, y_range (n_pc, 2) widened by one pixel, and the scales (simulations/_kikuchi_pattern_simulation.py:513-522)."""
    x_range, y_range = det.x_range.reshape(-1, 2), det.y_range.reshape(-1, 2)
    x_scale, y_scale = np.reshape(det.x_scale, -1), np.reshape(det.y_scale, -1)
    x_range[:, 0] -= x_scale
    x_range[:, 1] += x_scale
    y_range[:, 0] -= y_scale
    y_range[:, 1] += y_scale
    return x_range, y_range, x_scale, y_scale


def simulate(case, wrong=None):
    """The whole of on_detector for a case, navigation axes flattened: a dict of the kept lists and every array.
    `wrong`: "z_ge" (z >= 0 counts as upper), "not_widened" (bounds not widened by one pixel), "y_not_negated"."""
    det = detector(case)
    hkl, a_star = case["hkl"], case["basis"]
    q = case["rotations"].reshape(-1, 4)
    u_os = to_matrix(q) @ det.sample_to_detector.T
    a_direct = np.linalg.inv(a_star.T)
    upper = (lambda z: z >= 0) if wrong == "z_ge" else (lambda z: z > 0)
    hkl_d = np.matmul(hkl, np.matmul(a_star, u_os))
    keep = upper(hkl_d[..., 2]).any(axis=0)
    hkl_d = hkl_d[:, keep]
    uvw = zone_axes_brute_force(hkl[keep])
    uvw_d = np.matmul(uvw, np.matmul(a_direct, u_os))
    x_range, y_range, x_scale, y_scale = widened_ranges(det)
    if wrong == "not_widened":
        x_range, y_range = det.x_range.reshape(-1, 2), det.y_range.reshape(-1, 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        xg, yg = uvw_d[..., 0] / uvw_d[..., 2], uvw_d[..., 1] / uvw_d[..., 2]
        inside = ((xg >= x_range[:, :1]) & (xg <= x_range[:, 1:]) & (yg >= y_range[:, :1]) & (yg <= y_range[:, 1:]))
        keep_uvw = upper(uvw_d[..., 2]).any(axis=0) & inside.any(axis=0)
        uvw, uvw_d, xg, yg = uvw[keep_uvw], uvw_d[:, keep_uvw], xg[:, keep_uvw], yg[:, keep_uvw]
        r_max = float(np.max(det.r_max))
        pc = det.pc_flattened
        xoff, yoff = ((pc[:, 0] / pc[:, 2]) * det.aspect_ratio)[:, np.newaxis], (pc[:, 1] / pc[:, 2])[:, np.newaxis]
        xs, ys = x_scale[:, np.newaxis], y_scale[:, np.newaxis]
        sign = 1.0 if wrong == "y_not_negated" else -1.0
        # lines (simulations/_kikuchi_pattern_features.py:81-102; Vector3d.polar = arccos(z / r), .azimuth = arctan2(y, x) + 2 pi (< 0))
        x, y, z = hkl_d[..., 0], hkl_d[..., 1], hkl_d[..., 2]
        polar = np.arccos(z / np.sqrt(x**2 + y**2 + z**2))
        azimuth = np.arctan2(y, x)
        azimuth += (azimuth < 0) * 2 * np.pi
        hesse = np.tan(0.5 * np.pi - polar)
        within = (np.abs(hesse) < r_max) & (z > -1e-5)
        hesse_nan = np.where(within, hesse, np.nan)
        alpha = np.arccos(hesse_nan / r_max)
        a1, a2 = azimuth - np.pi + alpha, azimuth - np.pi - alpha
        line_gn = np.stack((np.cos(a1), np.sin(a1), np.cos(a2), np.sin(a2)), axis=-1) * r_max
        line_px = line_gn.copy()
        line_px[..., [0, 2]] = (line_px[..., [0, 2]] + xoff[..., np.newaxis]) / xs[..., np.newaxis]
        line_px[..., [1, 3]] = (sign * line_px[..., [1, 3]] + yoff[..., np.newaxis]) / ys[..., np.newaxis]
        # zone axes (simulations/_kikuchi_pattern_features.py:122-129, _kikuchi_pattern_simulation.py:494-532)
        r = np.sqrt(xg**2 + yg**2)
        zone_within = (r < r_max) & (uvw_d[..., 2] > -1e-5)
        zone_gn = np.where(zone_within[..., np.newaxis], np.stack((xg, yg), axis=-1), np.nan)
        gx, gy = zone_gn[..., 0], zone_gn[..., 1]
        zone_px = np.stack(((gx + xoff) / xs, (sign * gy + yoff) / ys), axis=-1)
        zone_inside = (gx >= x_range[:, :1]) & (gx <= x_range[:, 1:]) & (gy >= y_range[:, :1]) & (gy <= y_range[:, 1:])
        zone_px[~zone_inside] = np.nan
    return {"keep": keep, "uvw": uvw, "r_max": r_max, "x_scale": x_scale, "y_scale": y_scale,
            "x_range": x_range, "y_range": y_range, "hkl_d": hkl_d, "uvw_d": uvw_d,
            "line_in": upper(z), "line_within": within, "hesse_distance": hesse_nan, "hesse_alpha": alpha,
            "line_gn": line_gn, "line_px": line_px,
            "zone_in": upper(uvw_d[..., 2]), "zone_within": zone_within, "r_gnomonic": r, "zone_gn": zone_gn, "zone_px": zone_px}


def left_out(case, sim):
    """(lines (n, R), zone axes (n, Z)) pairs left out of a comparison with another evaluation: a line with
    | |t| - 1 | <= 1e-4, t = hesse distance / R_g; a pair with |z| or |z + 1e-5| below 1e-12 |v| (not in an `exact` case,
    whose hand-made z = 0 and z = -5e-6 are exact); a zone axis within 1e-9 of R_g or of a widened bound."""
    def near_z(v):
        norm = np.sqrt(np.sum(v**2, axis=-1))
        return (np.abs(v[..., 2]) < 1e-12 * norm) | (np.abs(v[..., 2] + 1e-5) < 1e-12 * norm)

    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, z = (sim["hkl_d"][..., i] for i in range(3))
        t = (z / np.sqrt(x**2 + y**2)) / sim["r_max"]
        lines = np.abs(np.abs(t) - 1) <= 1e-4
        xg, yg = sim["uvw_d"][..., 0] / sim["uvw_d"][..., 2], sim["uvw_d"][..., 1] / sim["uvw_d"][..., 2]
        zones = np.abs(np.sqrt(xg**2 + yg**2) - sim["r_max"]) <= 1e-9
        for g, rng in ((xg, sim["x_range"]), (yg, sim["y_range"])):
            zones |= (np.abs(g - rng[:, :1]) <= 1e-9) | (np.abs(g - rng[:, 1:]) <= 1e-9)
    if not case["exact"]:
        lines |= near_z(sim["hkl_d"])
        zones |= near_z(sim["uvw_d"])
    return lines, zones


def tolerances(sim):
    """atol of the gnomonic coordinates, and of the pixel x and y columns per point (n, 1): 1e-10 R_g, divided by the
    point's scale.  Rounding in the 3 x 3 chain moves a direction by about 20 eps; h = cot(polar) with |h| < R_g <~ 3
    amplifies that by 1 + h^2 <= 10; acos(t) by 1 / sqrt(1 - t^2) <= 71 for |t| <= 1 - 1e-4: about 1e-12 R_g, times 100."""
    atol = 1e-10 * sim["r_max"]
    return atol, (atol / sim["x_scale"])[:, np.newaxis], (atol / sim["y_scale"])[:, np.newaxis]


def compare(got, want, mask_out, atol):
    """Largest |got - want| over the pairs not left out, after asserting that NaN sits at the same places there.
    `got`, `want`: (n, f, c); `mask_out`: (n, f); `atol`: scalar or (n, 1) or (n, 1, c)."""
    use = ~mask_out
    g, w = got[use], want[use]
    assert np.array_equal(np.isnan(g), np.isnan(w)), "NaN at different places"
    with np.errstate(invalid="ignore"):
        err = np.where(g == w, 0.0, np.abs(g - w))  # (equal infinities: r_gnomonic at z = 0)
    tol = np.broadcast_to(atol, got.shape)[use]
    ok = np.isnan(w) | (err <= tol)
    worst = float(np.nanmax(err / tol)) if np.isfinite(err).any() else 0.0
    return bool(ok.all()), worst


def key(case, what):
    return f"{case['name']}__{what}"
