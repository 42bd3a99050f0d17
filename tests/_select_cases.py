"""The cases of tests/golden/select.npz, shared by tools/gen_select_golden.py (which runs the reference on them) and
tests/test_host_select.py: data only."""

import numpy as np

from kikuchipy_amd._selection import grid_indices

# (grid_shape, nav_shape): ints for 1-D maps, (rows, columns) else.  The first two are the reference's docstring cases;
# several return a smaller grid than the one asked for.
GRIDS = [
    ((4, 5), (55, 75)),
    (10, 105),
    ((3, 4), (55, 75)),
    ((2, 3), (7, 9)),
    ((3, 2), (7, 9)),
    ((1, 1), (7, 9)),
    ((5, 5), (6, 6)),
    ((6, 8), (7, 9)),
    ((2, 2), (13, 5)),
    ((10, 10), (100, 117)),
    ((3, 7), (20, 50)),
    (1, 7),
    (3, 7),
    (6, 7),
    (4, 65),
    (20, 130),
]

DETECTOR = dict(px_size=70.0, binning=2, tilt=5.0, azimuthal=1.5, sample_tilt=69.5)


def detector_pcs():
    """name -> (shape, pc): one PC, per-point PCs on a 2-D map and on a 1-D map."""
    rng = np.random.default_rng(20)
    return {
        "one": ((60, 60), np.array([[0.421, 0.779, 0.505]])),
        "one_wide": ((48, 64), np.array([[0.5, 0.5, 0.5]])),
        "map": ((60, 60), np.array([0.42, 0.78, 0.5]) + 0.02 * rng.random((3, 4, 3))),
        "line": ((12, 10), np.array([0.45, 0.7, 0.55]) + 0.01 * rng.random((5, 3))),
    }


# (top, bottom, left, right): inside, touching the edges, needing clamping, and refused (empty after clamping, reversed,
# not integers)
EXTENTS = [
    (10, 50, 5, 55),
    (0, 60, 0, 60),
    (0, 1, 0, 1),
    (3, 9, 2, 7),
    (-5, 30, -2, 20),
    (20, 1000, 30, 1000),
    (-10, 1000, -10, 1000),
    (30, 30, 0, 10),
    (40, 20, 0, 10),
    (0, 10, 50, 20),
    (1000, 2000, 0, 10),
    (0, 10, -20, -5),
    (1.0, 20, 0, 10),
    (0, 20.5, 0, 10),
]


# ---- the table of tests/test_gpu_select.py (tests/test_host_select.py checks select_plan.h's path for every entry)
DTYPES = ["uint8", "int8", "uint16", "int16", "float32", "float64"]
DETECTORS = [(3, 3), (5, 7), (12, 10), (16, 16)]
# 65 = one more than the most patterns select_plan.h puts into one workgroup (SEL_MAX_PATTERNS_PER_BLOCK): two
# workgroups for every detector here, three at 130
COUNTS = [1, 7, 65, 130]
MAPS = {1: (1, 1), 7: (7, 1), 65: (13, 5), 130: (13, 10)}


def probe(n, sy, sx, dtype):
    """Every element a unique function of (pattern, row, col): exact integers for the wide dtypes, for the 1-byte ones a
    multiplicative hash (no period that divides a row length)."""
    dt = np.dtype(dtype)
    lin = np.arange(n * sy * sx, dtype=np.uint64).reshape(n, sy, sx)
    if dt.itemsize == 1:
        return ((lin * np.uint64(2654435761) >> np.uint64(11)) & np.uint64(0xFF)).astype(np.uint8).view(dt)
    if dt.kind in "ui":
        return lin.astype(np.uint16).view(dt)  # (130 * 16 * 16 < 2^16: unique)
    return (lin + np.uint64(1)).astype(dt)


def rectangles(sy, sx):
    """(name, rows, cols) as (first, step, count)."""
    full_r, full_c = (0, 1, sy), (0, 1, sx)
    return [
        ("full", full_r, full_c),
        ("col0=1", full_r, (1, 1, sx - 1)),
        ("one column", full_r, (sx // 2, 1, 1)),
        ("one row", (sy // 2, 1, 1), full_c),
        ("last row and column", (sy - 1, 1, 1), (sx - 1, 1, 1)),
        ("rows 1:, full width", (1, 1, sy - 1), full_c),
        ("every 2nd row", (1, 2, len(range(1, sy, 2))), (1, 1, sx - 1)),
        ("steps 2 and 3", (0, 2, len(range(0, sy, 2))), (1, 3, len(range(1, sx, 3)))),
        ("steps 3 and 2", (1, 3, len(range(1, sy, 3))), (0, 2, len(range(0, sx, 2)))),
    ]


def index_lists(n):
    ny, nx = MAPS[n]
    lists = [("identity", None), ("reversed", np.arange(n)[::-1]), ("repeated", np.full(5, n // 2)),
             ("single", np.array([n - 1]))]
    if ny > 2 and nx > 2:
        g = grid_indices((2, 3), (ny, nx))
        lists.append(("extract_grid", (g[0] * nx + g[1]).ravel()))
    return lists
