"""Write tests/golden/geometrical.npz by RUNNING THE REFERENCE ITSELF: its `KikuchiPatternLine` and
`KikuchiPatternZoneAxis` (simulations/_kikuchi_pattern_features.py, loaded from the file) and the two methods
`_set_lines_detector_coordinates` / `_set_zone_axes_detector_coordinates` of `GeometricalKikuchiPatternSimulation`
(simulations/_kikuchi_pattern_simulation.py:468-534, executed from their source; the module as a whole needs Matplotlib,
HyperSpy and orix).  Test infrastructure; run it where the reference's sources are:

    python -W ignore tools/gen_geometrical_golden.py

orix is not installed.  `orix.vector` is replaced by a stand-in `Vector3d` with `x`, `y`, `z`, `polar` and `azimuth`
(orix/vector/vector3d.py: polar = arccos(z / radial), azimuth = arctan2(y, x), plus 2 pi where negative) and a `Miller`
that only has `ndim`.  The matrix chain of `on_detector` (simulations/kikuchi_pattern_simulator.py:254-353) that feeds the
classes is restated in NumPy here, with `Rotation.to_matrix` from tests/_geometrical_cases.py; the zone axes are the
reduced integer cross products in lexicographic order (orix' `Miller.round().unique()` order cannot be checked here).
The detector is this package's `EBSDDetector`, whose gnomonic quantities its own tests hold to the reference.

Only data goes in: the cases' inputs (hkl, reciprocal basis, quaternions, projection centres, detector parameters), the
expected arrays, the kept-index lists, the parameter names and defaults of the mirrored calls (`signatures`, read from
the reference's sources with `ast`), and `made_by`.  Cases: tests/_geometrical_cases.py."""

import ast
import json
import os
import platform
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _geometrical_cases as cases  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SIMULATION = "simulations/_kikuchi_pattern_simulation.py"


class Vector3d:
    """What the reference's feature classes read of orix' Vector3d (orix/vector/vector3d.py)."""

    def __init__(self, data):
        self.data = np.asarray(data, dtype=np.float64)

    x = property(lambda self: self.data[..., 0])
    y = property(lambda self: self.data[..., 1])
    z = property(lambda self: self.data[..., 2])

    @property
    def polar(self):
        return np.arccos(self.z / np.sqrt(np.sum(self.data**2, axis=-1)))

    @property
    def azimuth(self):
        azimuth = np.arctan2(self.y, self.x)
        azimuth += (azimuth < 0) * 2 * np.pi
        return azimuth


class Miller:
    def __init__(self, indices):
        self.indices = indices
        self.ndim = 1


def reference_classes():
    vector = types.ModuleType("orix.vector")
    vector.Miller, vector.Vector3d = Miller, Vector3d
    sys.modules.setdefault("orix", types.ModuleType("orix"))
    sys.modules["orix.vector"] = vector
    features = ref_shim._load("kikuchipy.simulations._kikuchi_pattern_features", "simulations/_kikuchi_pattern_features.py")
    return features.KikuchiPatternLine, features.KikuchiPatternZoneAxis


def reference_methods(names):
    """Methods of GeometricalKikuchiPatternSimulation, compiled from their source one by one."""
    path = os.path.join(ref_shim.SRC, SIMULATION)
    tree = ast.parse(open(path).read())
    klass = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GeometricalKikuchiPatternSimulation"][0]
    out = {}
    for node in klass.body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            node.returns = None
            for a in node.args.args:
                a.annotation = None
            g = {"np": np}
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), path, "exec"), g)
            out[node.name] = g[node.name]
    return out


def run_reference(case, line_cls, zone_cls, methods):
    """on_detector from :254 on for one case, navigation axes kept; the reference's classes do everything after the chain."""
    det = cases.detector(case)
    rot = case["rotations"]
    nav = rot.shape[:-1]
    hkl, a_star = case["hkl"], case["basis"]
    u_os = (cases.to_matrix(rot.reshape(-1, 4)) @ det.sample_to_detector.T).reshape(nav + (3, 3))
    hkl_d = np.matmul(hkl, np.matmul(a_star, u_os))
    nav_axes = tuple(range(len(nav)))
    hkl_is_upper = np.greater(np.atleast_2d(hkl_d[..., 2]), 0)
    hkl_in_a_pattern = ~np.isclose(np.sum(hkl_is_upper, axis=nav_axes), 0)
    hkl_in_pattern = hkl_is_upper[..., hkl_in_a_pattern]
    hkl_d = hkl_d[..., hkl_in_a_pattern, :]
    uvw = cases.zone_axes_brute_force(hkl[hkl_in_a_pattern])
    uvw_d = np.matmul(uvw, np.matmul(np.linalg.inv(a_star.T), u_os))
    uvw_is_upper = np.greater(np.atleast_2d(uvw_d[..., 2]), 0)
    uvw_in_a_pattern = ~np.isclose(np.sum(uvw_is_upper, axis=nav_axes), 0)
    uvw_xg = uvw_d[..., 0] / uvw_d[..., 2]
    uvw_yg = uvw_d[..., 1] / uvw_d[..., 2]
    x_range = det.x_range
    y_range = det.y_range
    x_scale = det.x_scale
    y_scale = det.y_scale
    x_range[..., 0] -= x_scale
    x_range[..., 1] += x_scale
    y_range[..., 0] -= y_scale
    y_range[..., 1] += y_scale
    x_range = np.expand_dims(x_range, axis=-2)
    y_range = np.expand_dims(y_range, axis=-2)
    within_x = np.logical_and(uvw_xg >= x_range[..., 0], uvw_xg <= x_range[..., 1])
    within_y = np.logical_and(uvw_yg >= y_range[..., 0], uvw_yg <= y_range[..., 1])
    within_gnomonic_bounds = np.any(within_x * within_y, axis=nav_axes)
    uvw_in_a_pattern = np.logical_and(uvw_in_a_pattern, within_gnomonic_bounds)
    uvw_in_pattern = uvw_is_upper[..., uvw_in_a_pattern]
    uvw_d = uvw_d[..., uvw_in_a_pattern, :]
    uvw = uvw[uvw_in_a_pattern]
    max_r_gnomonic = np.max(det.r_max)
    lines = line_cls(hkl=Miller(hkl[hkl_in_a_pattern]), hkl_detector=Vector3d(hkl_d), in_pattern=hkl_in_pattern,
                     max_r_gnomonic=max_r_gnomonic)
    zone_axes = zone_cls(uvw=Miller(uvw), uvw_detector=Vector3d(uvw_d), in_pattern=uvw_in_pattern,
                         max_r_gnomonic=max_r_gnomonic)
    sim = types.SimpleNamespace(detector=det, _lines=lines, _zone_axes=zone_axes)
    methods["_set_lines_detector_coordinates"](sim)
    methods["_set_zone_axes_detector_coordinates"](sim)
    n = int(np.prod(nav))
    return {"keep": hkl_in_a_pattern, "uvw": uvw,
            "line_in": lines.in_pattern.reshape(n, -1), "line_within": lines.within_r_gnomonic.reshape(n, -1),
            "hesse_distance": lines.hesse_distance.reshape(n, -1), "hesse_alpha": lines.hesse_alpha.reshape(n, -1),
            "line_gn": lines.plane_trace_coordinates.reshape(n, -1, 4), "line_px": sim._lines_detector_coordinates.reshape(n, -1, 4),
            "zone_in": zone_axes.in_pattern.reshape(n, -1), "zone_within": zone_axes.within_r_gnomonic.reshape(n, -1),
            "r_gnomonic": zone_axes.r_gnomonic.reshape(n, -1), "zone_gn": zone_axes._xy_within_r_gnomonic.reshape(n, -1, 2),
            "zone_px": sim._zone_axes_detector_coordinates.reshape(n, -1, 2)}


STORED = ("keep", "uvw", "line_in", "line_within", "hesse_distance", "hesse_alpha", "line_gn", "line_px", "zone_in",
          "zone_within", "r_gnomonic", "zone_gn", "zone_px")


def signatures():
    """Parameter names and literal defaults of the mirrored calls, read from the reference's sources: a JSON string
    {call: [[name, default or "<required>"], ...]} (self left out)."""
    wanted = {"simulations/kikuchi_pattern_simulator.py": ("KikuchiPatternSimulator", ("on_detector",)),
              SIMULATION: ("GeometricalKikuchiPatternSimulation",
                           ("lines_coordinates", "zone_axes_coordinates", "as_collections", "as_markers", "plot"))}
    table = {}
    for rel, (cls, names) in wanted.items():
        tree = ast.parse(open(os.path.join(ref_shim.SRC, rel)).read())
        klass = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0]
        for node in klass.body:
            if isinstance(node, ast.FunctionDef) and node.name in names:
                args = node.args.args[1:]
                defaults = [None] * (len(args) - len(node.args.defaults)) + list(node.args.defaults)
                assert not node.args.kwonlyargs and node.args.vararg is None and node.args.kwarg is None
                table[f"{cls}.{node.name}"] = [[a.arg, "<required>" if d is None else ast.literal_eval(d)]
                                               for a, d in zip(args, defaults)]
    return json.dumps(table, sort_keys=True)


def main():
    line_cls, zone_cls = reference_classes()
    methods = reference_methods(("_set_lines_detector_coordinates", "_set_zone_axes_detector_coordinates"))
    out = {"made_by": np.array("the reference's KikuchiPatternLine / KikuchiPatternZoneAxis / _set_*_detector_coordinates "
                               f"under python {platform.python_version()}, numpy {np.__version__}"),
           "signatures": np.array(signatures())}
    with np.errstate(all="ignore"):
        for case in cases.cases():
            for name in ("hkl", "basis", "rotations", "pc"):
                out[cases.key(case, "in_" + name)] = np.asarray(case[name], dtype=np.float64)
            out[cases.key(case, "in_det")] = np.array(json.dumps(case["det"], sort_keys=True))
            if not case["golden"]:
                continue
            ref = run_reference(case, line_cls, zone_cls, methods)
            for name in STORED:
                out[cases.key(case, name)] = ref[name]
            mine = cases.simulate(case)
            lines_out, zones_out = cases.left_out(case, mine)
            print(case["name"], "lines", ref["line_gn"].shape, "zone axes", ref["zone_gn"].shape, "kept lists equal:",
                  np.array_equal(mine["keep"], ref["keep"]) and np.array_equal(mine["uvw"], ref["uvw"]),
                  "left out:", int(lines_out.sum()), int(zones_out.sum()), flush=True)
    path = os.path.join(GOLDEN, "geometrical.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
