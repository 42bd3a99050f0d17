"""Write tests/golden/select.npz by RUNNING THE REFERENCE ITSELF: its `grid_indices` (signals/util/array_tools.py:21-107,
the function executed from its source) and its `EBSDDetector.crop` (detectors/_ebsd_detector.py:986-1032, the method
executed from its source on a stand-in detector - the module as a whole needs orix and Matplotlib).  Test
infrastructure; run it where the reference's sources are:

    python -W ignore tools/gen_select_golden.py

Only data goes in: per case the inputs, and the indices and spacing, or the cropped shape and PCs, or the text of the
ValueError the reference raised.  Cases: tests/_select_cases.py."""

import ast
import os
import platform
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _select_cases as cases  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


class Detector:
    """What the reference's `crop` reads of its detector, and what it builds the new one from."""

    def __init__(self, shape, pc, tilt, sample_tilt, binning, px_size, azimuthal):
        self.shape, self.pc = tuple(shape), np.asarray(pc, dtype=np.float64)
        self.tilt, self.sample_tilt, self.px_size, self.azimuthal = tilt, sample_tilt, px_size, azimuthal
        self._binning = binning

    pcx = property(lambda self: self.pc[..., 0])
    pcy = property(lambda self: self.pc[..., 1])
    pcz = property(lambda self: self.pc[..., 2])


def reference_crop():
    path = os.path.join(ref_shim.SRC, "detectors/_ebsd_detector.py")
    tree = ast.parse(open(path).read())
    klass = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "EBSDDetector"][0]
    node = [n for n in klass.body if isinstance(n, ast.FunctionDef) and n.name == "crop"][0]
    node.returns = None
    for a in node.args.args:
        a.annotation = None
    g = {"np": np}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[node], type_ignores=[])), path, "exec"), g)
    return g["crop"]


def main():
    grid_indices = ref_shim.load_function_source("signals/util/array_tools.py", "grid_indices")
    crop = reference_crop()
    out = {"made_by": np.array("the reference's grid_indices and EBSDDetector.crop under python "
                               f"{platform.python_version()}, numpy {np.__version__}")}
    for i, (grid, nav) in enumerate(cases.GRIDS):
        idx, spacing = grid_indices(grid, nav, return_spacing=True)
        out[f"grid__{i}__idx"] = np.asarray(idx)
        out[f"grid__{i}__spacing"] = np.asarray(spacing)
        print("grid", grid, "in", nav, "->", idx.shape[1:], "spacing", spacing)
    d = cases.DETECTOR
    for name, (shape, pc) in cases.detector_pcs().items():
        for j, extent in enumerate(cases.EXTENTS):
            det = Detector(shape, pc, d["tilt"], d["sample_tilt"], d["binning"], d["px_size"], d["azimuthal"])
            try:
                new = crop(det, extent)
            except ValueError as e:
                out[f"crop__{name}__{j}__error"] = np.array(str(e))
                print("crop", name, extent, "refused")
                continue
            out[f"crop__{name}__{j}__shape"] = np.array(new.shape)
            out[f"crop__{name}__{j}__pc"] = np.asarray(new.pc, dtype=np.float64).reshape(-1, 3)
            assert (new.tilt, new.sample_tilt, new._binning, new.px_size, new.azimuthal) == \
                (d["tilt"], d["sample_tilt"], d["binning"], d["px_size"], d["azimuthal"])
            print("crop", name, extent, "->", new.shape)
    path = os.path.join(GOLDEN, "select.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", out["made_by"])


if __name__ == "__main__":
    main()
