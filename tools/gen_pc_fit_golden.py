"""Write tests/golden/pc_fit.npz by RUNNING THE REFERENCE ITSELF: the functions of detectors/_fit_projection_center.py
(loaded from the file) and the methods `extrapolate_pc`, `_pc_bruker2emsoft`, `_pc_bruker2tsl` and `_pc_bruker2oxford` of
its `EBSDDetector` (detectors/_ebsd_detector.py, compiled from their source one by one; the module as a whole needs
Matplotlib and orix).  Test infrastructure; run it where the reference's sources are, with the interpreter that has
scikit-learn 0.24.2 and scikit-image 0.18.3:

    python3.9 -W ignore tools/gen_pc_fit_golden.py

orix is not installed.  `orix.quaternion.Rotation` and `orix.vector.Vector3d` are replaced by stand-ins written here, in
quaternion arithmetic (v' = q v q*; the package under test uses matrices): `from_axes_angles`, the products with a
rotation and with a vector, `~`, and of the vector `data`, `unit`, `z`, `-`, `+`, `zvector`.  `kikuchipy._constants`
gets a `dependency_version` read from the installed scikit-image, and the detector the functions take is this package's
`EBSDDetector`, whose attributes its own tests hold to the reference.

Only data goes in: the cases' inputs, the reference's outputs, the parameter names and defaults of the mirrored methods
(`signatures`, read from the reference's source with `ast`), and `made_by`.  The robust case is kept only if
`RANSACRegressor` names the same outliers under every one of 20 seeds AND the all-pairs rule of kikuchipy_amd/_pc_fit.py
names them too: where the two could differ there is nothing to hold the package to.  A fit case is kept only if the
reference's fitted PCs lie within 0.01 of the PCs it was given."""

import ast
import json
import os
import platform
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DETECTOR = "detectors/_ebsd_detector.py"
N_SEEDS = 20
MISFIT = 0.01  # PCs are of order 1 and scattered by 2e-4


# ---- stand-ins ------------------------------------------------------------------------------------------------------------
class Vector3d:
    def __init__(self, data):
        self.data = np.atleast_2d(np.asarray(data.data if isinstance(data, Vector3d) else data, dtype=np.float64))

    x = property(lambda self: self.data[..., 0])
    y = property(lambda self: self.data[..., 1])
    z = property(lambda self: self.data[..., 2])

    @property
    def unit(self):
        return Vector3d(self.data / np.sqrt(np.sum(self.data**2, axis=-1, keepdims=True)))

    @classmethod
    def zvector(cls):
        return cls([0.0, 0.0, 1.0])

    def __neg__(self):
        return Vector3d(-self.data)

    def __sub__(self, other):
        return Vector3d(self.data - other.data)

    def __add__(self, other):
        return Vector3d(self.data + other.data)


class Rotation:
    """A unit quaternion (a, b, c, d); `rot * v` turns v by the angle about the axis: v' = q v q*."""

    def __init__(self, q):
        self.q = np.asarray(q, dtype=np.float64)

    @classmethod
    def from_axes_angles(cls, axis, angle):
        axis = np.asarray(axis, dtype=np.float64)
        axis = axis / np.sqrt(np.sum(axis**2))
        return cls(np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis]))

    def __invert__(self):
        return Rotation(self.q * np.array([1.0, -1.0, -1.0, -1.0]))

    def __mul__(self, other):
        a, b, c, d = self.q
        if isinstance(other, Rotation):
            e, f, g, h = other.q
            return Rotation([a * e - b * f - c * g - d * h, a * f + b * e + c * h - d * g,
                             a * g - b * h + c * e + d * f, a * h + b * g - c * f + d * e])
        x, y, z = other.data[..., 0], other.data[..., 1], other.data[..., 2]
        # orix/quaternion/quaternion.py, qu_rotate_vec: v' = q v q*
        return Vector3d(np.stack([(a**2 + b**2 - c**2 - d**2) * x + 2 * ((a * c + b * d) * z + (b * c - a * d) * y),
                                  (a**2 - b**2 + c**2 - d**2) * y + 2 * ((a * d + b * c) * x + (c * d - a * b) * z),
                                  (a**2 - b**2 - c**2 + d**2) * z + 2 * ((a * b + c * d) * y + (b * d - a * c) * x)], axis=-1))


def reference_functions():
    import skimage
    from packaging.version import Version

    import kikuchipy_amd as kpa

    quaternion, vector = types.ModuleType("orix.quaternion"), types.ModuleType("orix.vector")
    quaternion.Rotation, vector.Vector3d = Rotation, Vector3d
    sys.modules.setdefault("orix", types.ModuleType("orix"))
    sys.modules["orix.quaternion"], sys.modules["orix.vector"] = quaternion, vector
    ref_shim._ns("kikuchipy", ref_shim.SRC)
    constants = types.ModuleType("kikuchipy._constants")
    constants.dependency_version = {"scikit-image": Version(skimage.__version__)}
    sys.modules["kikuchipy._constants"] = constants
    ref_shim._ns("kikuchipy.detectors", os.path.join(ref_shim.SRC, "detectors"))
    detector = types.ModuleType("kikuchipy.detectors._ebsd_detector")
    detector.EBSDDetector = kpa.EBSDDetector
    sys.modules["kikuchipy.detectors._ebsd_detector"] = detector
    return ref_shim._load("kikuchipy.detectors._fit_projection_center", "detectors/_fit_projection_center.py")


def detector_class_node():
    tree = ast.parse(open(os.path.join(ref_shim.SRC, DETECTOR)).read())
    return [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "EBSDDetector"][0]


def reference_methods(names):
    """Methods of the reference's EBSDDetector, compiled from their source one by one (the last definition of a name:
    the ones before it are `@overload` stubs)."""
    from copy import deepcopy

    out = {}
    for node in detector_class_node().body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            node.returns, node.decorator_list = None, []
            for a in node.args.args:
                a.annotation = None
            g = {"np": np, "deepcopy": deepcopy}
            exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), DETECTOR, "exec"), g)
            out[node.name] = g[node.name]
    return out


METHODS = ("estimate_xtilt", "estimate_xtilt_ztilt", "extrapolate_pc", "fit_pc", "pc_emsoft", "pc_bruker", "pc_tsl", "pc_oxford")


def signatures():
    table = {}
    for node in detector_class_node().body:
        if isinstance(node, ast.FunctionDef) and node.name in METHODS:
            args = node.args.args[1:]
            defaults = [None] * (len(args) - len(node.args.defaults)) + list(node.args.defaults)
            assert not node.args.kwonlyargs and node.args.vararg is None and node.args.kwarg is None
            table[node.name] = [[a.arg, "<required>" if d is None else ast.literal_eval(d)] for a, d in zip(args, defaults)]
    return json.dumps(table, sort_keys=True)


# ---- cases ----------------------------------------------------------------------------------------------------------------
SAMPLE_TILT, TILT, SHAPE, PX_SIZE, STEP = 70.0, 3.0, (60, 60), 70.0, 1.5


def plane_pcs(rows, cols, rng, scatter=2e-4):
    """PCs of map points (rows, cols) on the plane of a sample tilted 70 degrees before a detector tilted 3, with Gaussian
    scatter."""
    alpha = np.deg2rad(90 - SAMPLE_TILT + TILT)
    f = STEP / (PX_SIZE * SHAPE[0])
    pc = np.stack([0.52 - cols * f, 0.21 + rows * f * np.cos(alpha), 0.55 - rows * f * np.sin(alpha)], axis=-1)
    return pc + scatter * rng.standard_normal(pc.shape)


def grids():
    rng = np.random.default_rng(20260101)
    r5, c5 = np.meshgrid(np.arange(5) * 10.0, np.arange(5) * 10.0, indexing="ij")
    out5 = np.zeros((5, 5), dtype=bool)
    out5[1, 3] = out5[4, 0] = True
    c7 = np.arange(7) * 6.0
    out7 = np.zeros(7, dtype=bool)
    out7[2] = True
    my, mx = np.indices((41, 41))
    return {
        "g5": dict(pc=plane_pcs(r5, c5, rng), pc_indices=np.stack([r5, c5]).astype(int), is_outlier=out5,
                   map2=np.stack([my.ravel(), mx.ravel()])[:, ::7], map3=np.stack([my, mx])[:, ::5, ::4]),
        "g7": dict(pc=plane_pcs(np.zeros(7), c7, rng), pc_indices=np.stack([np.zeros(7), c7]).astype(int), is_outlier=out7,
                   map2=np.stack([np.zeros(37, dtype=int), np.arange(37)]), map3=np.stack([np.zeros((1, 37), dtype=int), np.arange(37)[None]])),
    }


def main():
    import kikuchipy_amd as kpa
    from kikuchipy_amd import _pc_fit

    ref = reference_functions()
    methods = reference_methods(("extrapolate_pc", "_pc_bruker2emsoft", "_pc_bruker2tsl", "_pc_bruker2oxford"))
    import skimage
    import sklearn

    out = {"made_by": np.array("the reference's detectors/_fit_projection_center.py and EBSDDetector.extrapolate_pc / _pc_bruker2* "
                               f"under python {platform.python_version()}, numpy {np.__version__}, scikit-learn "
                               f"{sklearn.__version__}, scikit-image {skimage.__version__}"),
           "signatures": np.array(signatures()),
           "detector": np.array(json.dumps(dict(shape=SHAPE, px_size=PX_SIZE, sample_tilt=SAMPLE_TILT, tilt=TILT)))}
    fits = []
    for name, g in grids().items():
        det = kpa.EBSDDetector(SHAPE, px_size=PX_SIZE, sample_tilt=SAMPLE_TILT, tilt=TILT, pc=g["pc"])
        for key in ("pc", "pc_indices", "is_outlier", "map2", "map3"):
            out[f"{name}_{key}"] = g[key]
        for transformation in ("projective", "affine"):
            for map_form in ("map2", "map3"):
                for masked in (False, True):
                    case = f"{name}_{transformation}_{map_form}_{'masked' if masked else 'all'}"
                    try:
                        with np.errstate(all="ignore"):
                            pc_fit, pc_map, pc_used, x_tilt, intercept, slope = ref.fit_plane_to_pc(
                                detector=det, pc_indices=g["pc_indices"], map_indices=g[map_form],
                                is_outlier=g["is_outlier"] if masked else None, transformation=transformation)
                        # a fit that does not come back to the PCs it was given is no fit: the projective one of a 1-D
                        # grid, whose homography is not determined (scikit-image reports failure, the reference goes on
                        # with the identity)
                        ok = bool(np.all(np.isfinite(pc_map)) and np.isfinite(x_tilt) and np.abs(pc_fit - pc_used).max() < MISFIT)
                    except Exception as e:  # noqa: BLE001 - whatever the reference raises is recorded as "no result"
                        print(case, "the reference raised", type(e).__name__, e)
                        ok = False
                    if not ok:
                        print(case, "NOT STORED: the reference has no result within", MISFIT, "of the PCs")
                        continue
                    out[case + "_pc"], out[case + "_xtilt"] = pc_map, np.float64(x_tilt)
                    fits.append(case)
        out[name + "_xtilt_linear"] = np.float64(ref.estimate_xtilt_linear(detector=det)[0])
        for masked in (False, True):
            pc = det.pc[~g["is_outlier"]] if masked else det.pc
            pc = pc.reshape((-1, 3))
            x_tilt, z_tilt, *_ = ref.fit_hyperplane(pc - pc.mean(axis=0))
            out[f"{name}_xz_{'masked' if masked else 'all'}"] = np.array([x_tilt, z_tilt], dtype=np.float64)
    out["fit_cases"] = np.array(json.dumps(fits))

    # the robust fit: three PCy values displaced well beyond the threshold
    g = grids()["g5"]
    pc = g["pc"].copy()
    for (i, j), d in zip(((0, 2), (2, 4), (3, 1)), (0.02, 0.03, 0.04)):
        pc[i, j, 1] += d
    det = kpa.EBSDDetector(SHAPE, px_size=PX_SIZE, sample_tilt=SAMPLE_TILT, tilt=TILT, pc=pc)
    seen = []
    for seed in range(N_SEEDS):
        np.random.seed(seed)
        x_tilt, _, is_outlier = ref.estimate_xtilt_linear_robust(detector=det)
        seen.append((x_tilt, is_outlier.copy()))
    slope, _, inlier = _pc_fit.robust_linear_fit(det.pcz.ravel(), det.pcy.ravel())
    agree = all(np.array_equal(m, seen[0][1]) for _, m in seen) and np.array_equal(~inlier, seen[0][1])
    print("robust case:", int(seen[0][1].sum()), "outliers; all", N_SEEDS, "seeds and the all-pairs rule agree:", agree,
          "; tilt spread over the seeds", np.ptp([t for t, _ in seen]), "; all-pairs tilt minus the reference's",
          float(np.pi / 2 + np.arctan(slope)) - seen[0][0])
    if agree:
        out["robust_pc"], out["robust_is_outlier"], out["robust_xtilt"] = pc, seen[0][1].reshape(5, 5), np.float64(seen[0][0])

    # extrapolate_pc: indices outside the map, and shape / px_size / binning given
    det = kpa.EBSDDetector(SHAPE, px_size=PX_SIZE, sample_tilt=SAMPLE_TILT, tilt=TILT, pc=g["pc"])
    indices = g["pc_indices"].reshape(2, -1) - np.array([[15], [-30]])  # rows from -15, columns up to 70: outside a 31 x 41 map
    out["extrapolate_indices"] = indices
    for case, kwargs in (("plain", {}), ("given", dict(shape=(120, 100), px_size=35.0, binning=2)),
                         ("masked", dict(is_outlier=g["is_outlier"].ravel()))):
        new = methods["extrapolate_pc"](det, indices, (31, 41), (1.5, 2.0), **kwargs)
        out[f"extrapolate_{case}_pc"] = new.pc
        out[f"extrapolate_{case}_detector"] = np.array(json.dumps(dict(shape=new.shape, px_size=new.px_size, binning=new.binning)))

    # the conventions: a detector that is not square, binned, with a pixel size
    det = kpa.EBSDDetector((60, 80), px_size=59.2, binning=8, pc=g["pc"])
    out["convention_detector"] = np.array(json.dumps(dict(shape=(60, 80), px_size=59.2, binning=8)))
    out["convention_emsoft4"] = methods["_pc_bruker2emsoft"](det, version=4)
    out["convention_emsoft5"] = methods["_pc_bruker2emsoft"](det, version=5)
    out["convention_tsl"] = methods["_pc_bruker2tsl"](det)
    out["convention_oxford"] = methods["_pc_bruker2oxford"](det)
    tall = kpa.EBSDDetector((80, 60), pc=g["pc"])
    out["convention_tall_tsl"], out["convention_tall_oxford"] = methods["_pc_bruker2tsl"](tall), methods["_pc_bruker2oxford"](tall)

    path = os.path.join(GOLDEN, "pc_fit.npz")
    np.savez_compressed(path, **out)
    print("stored fits:", fits)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
