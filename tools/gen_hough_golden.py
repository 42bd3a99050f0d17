"""Write tests/golden/hough_ni.npz: the Bunge angles (radians) of the `CrystalMap` that the reference's nine experimental
Ni patterns come with - `Scan 1/EBSD/Data/{phi1, Phi, phi2}` of its data/kikuchipy_h5ebsd/patterns.h5 - the known answer
of the Hough indexing tests (tests/_hough_cases.py: ni_experimental).  Only data goes in.

    python tools/gen_hough_golden.py /path/to/kikuchipy/data/kikuchipy_h5ebsd/patterns.h5

Needs h5py.  RECORDED holds the values as the file gives them to eight decimals; the script refuses to write anything
that differs from them, and without h5py or without a path it writes them as they stand."""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "hough_ni.npz")
RECORDED = {
    "phi1": [4.50142171, 5.09304897, 5.09171357, 6.08375679, 5.09182627, 5.08948563, 4.50207689, 5.08526435, 3.53372654],
    "Phi": [0.99720894, 1.07741137, 1.07938329, 1.55065387, 1.08271934, 1.08436952, 0.99156558, 1.08577579, 1.58835474],
    "phi2": [1.59252632, 3.16027762, 3.15638304, 2.57002697, 3.15660981, 3.15320701, 0.02215707, 0.01307323, 0.49216135],
}


def main(argv):
    angles = {k: np.array(v) for k, v in RECORDED.items()}
    try:
        import h5py
    except ImportError:
        h5py = None
    if h5py is not None and len(argv) > 1:
        with h5py.File(argv[1], "r") as f:
            data = f["Scan 1/EBSD/Data"]
            read = {k: np.asarray(data[k], dtype=np.float64).reshape(-1) for k in RECORDED}
        for k in RECORDED:
            if read[k].shape != angles[k].shape or np.abs(read[k] - angles[k]).max() > 5e-9:
                raise SystemExit(f"{k} of {argv[1]} is not the recorded column: {read[k]}")
        angles = read
    np.savez(OUT, source=np.array("Scan 1/EBSD/Data/{phi1,Phi,phi2} of kikuchipy's data/kikuchipy_h5ebsd/patterns.h5, radians"),
             **angles)
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv)
