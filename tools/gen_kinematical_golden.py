"""Write tests/golden/kinematical.npz by RUNNING THE REFERENCE ITSELF: its `get_pattern`
(simulations/kikuchi_pattern_simulator.py:685-700, executed from the file with Numba stubbed to plain Python, `vec_dot` of
_utils/numba.py and `poles_from_hemisphere` of _utils/vector.py beside it) the way `calculate_master_pattern` (:162-199)
calls it, and `_lambert2vector` (signals/util/_master_pattern.py) with `scipy.interpolate.interpn` under the arguments of
`KikuchiMasterPattern.as_lambert` (signals/_kikuchi_master_pattern.py:166-205), verbatim.  Test infrastructure; run it
where the reference's sources are, with an interpreter that knows `match` (_utils/vector.py uses it):

    python3.10 -W ignore tools/gen_kinematical_golden.py

orix is not installed, so the two one-line orix formulas between those functions are restated here (and in
tests/_kinematical_cases.py) with their source: `InverseStereographicProjection(pole).xy2vector` and
`StereographicProjection().vector2xy` of orix/projections/stereographic.py.

Only data goes in: the cases' inputs (unit vectors, Bragg angles, structure factors), the master patterns, the Lambert
pattern of the end-to-end case, the parameter names and defaults of the mirrored calls (`signatures`, read from the
reference's sources), and the versions that made them (`made_by`).  Cases: tests/_kinematical_cases.py."""

import os
import platform
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _kinematical_cases as cases  # noqa: E402
import _kinematical_restate as restate  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


class _Signature:
    """Stands in for `nb.float64` in get_pattern's decorator: `nb.float64[:](nb.float64[:], ...)`."""

    def __getitem__(self, item):
        return self

    def __call__(self, *args):
        return self


def reference_functions():
    ref = ref_shim.load_reference_projection()
    ref_shim._load("kikuchipy._utils.exceptions", "_utils/exceptions.py")
    vector = ref_shim._load("kikuchipy._utils.vector", "_utils/vector.py")
    nb = types.SimpleNamespace(njit=sys.modules["numba"].njit, prange=range, float64=_Signature())
    get_pattern = ref_shim.load_function_source("simulations/kikuchi_pattern_simulator.py", "get_pattern",
                                                {"nb": nb, "vec_dot": ref["numba_utils"].vec_dot})
    return get_pattern, vector.poles_from_hemisphere, ref["master_pattern"]._lambert2vector


def xy2vector(pole, x, y):
    """orix/projections/stereographic.py, InverseStereographicProjection.xy2vector"""
    denom = 1 + x**2 + y**2
    return np.column_stack([2 * x / denom, 2 * y / denom, -pole * (1 - x**2 - y**2) / denom])


def vector2xy(xyz):
    """orix/projections/stereographic.py, StereographicProjection.vector2xy with the default pole -1"""
    return xyz[:, 0] / (1 + xyz[:, 2]), xyz[:, 1] / (1 + xyz[:, 2])


def master_pattern(case, get_pattern, poles_from_hemisphere):
    """simulations/kikuchi_pattern_simulator.py:165-199"""
    u, theta, f = cases.reflectors(case["reflectors"], case["m"])
    intensity = cases.intensity(f, case["scaling"])
    size = int(2 * case["half_size"] + 1)
    poles = poles_from_hemisphere(case["hemisphere"])
    arr = np.linspace(-1, 1, size)
    X, Y = np.meshgrid(arr, arr)
    X = X.ravel()
    Y = Y.ravel()
    patterns = np.empty((len(poles), size * size), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for i in range(len(poles)):
            xyz_hemi = xy2vector(poles[i], X.ravel(), Y.ravel())
            patterns[i] = get_pattern(intensity, xyz_hemi, u, theta)
    patterns = patterns.reshape(-1, size, size)  # (the reference squeezes here; a 1 x 1 pattern keeps its axes)
    return patterns if case["hemisphere"] == "both" else patterns[0]


def as_lambert(data, lambert2vector):
    """signals/_kikuchi_master_pattern.py:166-205"""
    from scipy.interpolate import interpn

    sig_shape = data.shape[-2:]
    arr = np.linspace(-1, 1, sig_shape[0], dtype=np.float64)
    x_lambert, y_lambert = np.meshgrid(arr, arr)
    x_lambert_flat = x_lambert.ravel()
    y_lambert_flat = y_lambert.ravel()
    xyz_upper = lambert2vector(x_lambert_flat, y_lambert_flat)
    x_stereo, y_stereo = vector2xy(xyz_upper)
    x_stereo += 1
    y_stereo += 1
    kwargs = {
        "points": (arr + 1, arr + 1),
        "xi": (y_stereo, x_stereo),
        "method": "splinef2d",
    }
    data_out = np.zeros(data.shape, dtype=np.float32)
    for idx in np.ndindex(data.shape[:-2]):
        data_i = interpn(values=data[idx], **kwargs)
        data_out[idx] = data_i.reshape(sig_shape)
    return data_out


def signatures():
    """Parameter names and literal defaults of the three mirrored calls, read from the reference's sources: a JSON
    string {call: [[name, default or "<required>"], ...]} (self left out)."""
    import ast
    import json

    wanted = {"simulations/kikuchi_pattern_simulator.py": ("KikuchiPatternSimulator", ("__init__", "calculate_master_pattern")),
              "signals/_kikuchi_master_pattern.py": ("KikuchiMasterPattern", ("as_lambert",))}
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
    import scipy

    get_pattern, poles_from_hemisphere, lambert2vector = reference_functions()
    out = {"made_by": np.array(f"the reference's get_pattern / _lambert2vector / interpn(splinef2d) under python "
                               f"{platform.python_version()}, numpy {np.__version__}, scipy {scipy.__version__}")}
    for which in ("ni", "handmade"):
        u, theta, f = cases.reflectors(which)
        out[f"in__{which}__unit_vectors"], out[f"in__{which}__theta"], out[f"in__{which}__structure_factor"] = u, theta, f
    out["in__ni__hkl"] = cases.ni_reflectors()[0]
    out["signatures"] = np.array(signatures())
    left = 0
    for case in cases.cases() + [cases.END_TO_END]:
        if not case["golden"]:
            continue
        ref = master_pattern(case, get_pattern, poles_from_hemisphere)
        out[cases.key(case)] = ref
        mine = restate.master_pattern(case)
        near = int(restate.left_out(case).sum())
        left += near
        print(cases.key(case), ref.shape, "restatement equal:", np.array_equal(mine, ref), "near a threshold:", near, flush=True)
    print("pixels within 1e-12 of a threshold, all cases:", left)
    out["lambert__" + cases.END_TO_END["name"]] = as_lambert(out[cases.key(cases.END_TO_END)], lambert2vector)
    path = os.path.join(GOLDEN, "kinematical.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
