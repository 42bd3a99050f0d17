"""Selecting data without a GPU: `grid_indices` and `EBSDDetector.crop` against the reference's own results
(tests/golden/select.npz, made by tools/gen_select_golden.py), the translation of HyperSpy-order keys into pattern
indices and detector rectangles against NumPy indexing, the kernel path choice (csrc/select_plan.h compiled with the
host compiler) for every case of the GPU table, the signatures of the new methods, and `inav` / `isig` / `crop` /
`crop_signal` / `extract_grid` on host-backed signals, including the equalities of the reference's example scripts."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import _select_cases as cases
import kikuchipy_amd as kpa
from conftest import ROOT
from kikuchipy_amd import _selection
from kikuchipy_amd.detectors import EBSDDetector

G = np.load(os.path.join(ROOT, "tests", "golden", "select.npz"))


# ---------------------------------------------------------------- the reference's results
def test_grid_indices_equal_the_reference():
    differs = 0
    for i, (grid, nav) in enumerate(cases.GRIDS):
        idx, spacing = _selection.grid_indices(grid, nav, return_spacing=True)
        want = G[f"grid__{i}__idx"]
        assert idx.shape == want.shape and np.array_equal(idx, want), (grid, nav)
        assert np.array_equal(spacing, G[f"grid__{i}__spacing"]), (grid, nav)
        assert np.array_equal(_selection.grid_indices(grid, nav), want)
        asked = (grid,) if isinstance(grid, int) else tuple(grid)
        differs += idx.shape[1:] != asked
    assert differs >= 3  # grids that come back smaller than asked for are among the cases
    # the reference's docstring cases
    assert _selection.grid_indices((4, 5), (55, 75))[:, 0, 0].tolist() == [11, 12]
    assert _selection.grid_indices(10, 105).tolist() == [[8, 18, 28, 38, 48, 58, 68, 78, 88, 98]]
    with pytest.raises(ValueError, match="must both signify either a 1D or 2D grid"):
        _selection.grid_indices((2, 2), 10)


def test_detector_crop_equals_the_reference():
    d = cases.DETECTOR
    cropped = refused = 0
    for name, (shape, pc) in cases.detector_pcs().items():
        for j, extent in enumerate(cases.EXTENTS):
            det = EBSDDetector(shape=shape, pc=pc, twist=0.5, **d)
            key = f"crop__{name}__{j}__"
            if key + "error" in G:
                with pytest.raises(ValueError) as e:
                    det.crop(extent)
                assert str(e.value) == str(G[key + "error"])
                refused += 1
                continue
            new = det.crop(extent)
            assert new.shape == tuple(G[key + "shape"]), (name, extent)
            want = G[key + "pc"]
            assert np.array_equal(new.pc.reshape(-1, 3), want), (name, extent)  # the same three operations: the same bits
            assert new.navigation_shape == det.navigation_shape
            assert (new.tilt, new.sample_tilt, new.binning, new.px_size, new.azimuthal) == \
                (d["tilt"], d["sample_tilt"], d["binning"], d["px_size"], d["azimuthal"])
            assert new.twist == 0.5
            assert det.shape == tuple(shape) and np.array_equal(det.pc.reshape(-1, 3), np.reshape(pc, (-1, 3)))
            cropped += 1
    assert cropped >= 20 and refused >= 20


# ---------------------------------------------------------------- keys -> (pattern_index, rectangle)
NAV_KEYS = [slice(None), 0, -1, 3, slice(1, None), slice(None, -2), slice(1, 6, 2), slice(-4, None, 3), slice(2, 3),
            slice(0, 100), slice(None, None, 4)]


@pytest.mark.parametrize("nav", [(7, 9), (9,), (1, 9), (7, 1)])
def test_navigation_keys_against_numpy(nav):
    flat_index = np.arange(int(np.prod(nav))).reshape(nav)
    keys = NAV_KEYS if len(nav) == 1 else [(kx, ky) for kx in NAV_KEYS for ky in NAV_KEYS] + NAV_KEYS
    n = 0
    for key in keys:
        per_axis = (key if isinstance(key, tuple) else (key,)) + (slice(None),) * len(nav)
        per_axis = per_axis[:len(nav)][::-1]  # HyperSpy's (x, y) -> the array's (rows, columns)
        try:
            want = flat_index[per_axis]
        except IndexError:
            with pytest.raises(IndexError):
                _selection.navigation_selection(nav, key)
            continue
        if want.size == 0:
            with pytest.raises(IndexError, match="selects nothing"):
                _selection.navigation_selection(nav, key)
            continue
        flat, new_nav, axes = _selection.navigation_selection(nav, key)
        assert flat.dtype == np.int64 and new_nav == want.shape and np.array_equal(flat, want.ravel()), (nav, key)
        assert [a[3] for a in axes] == [isinstance(k, int) for k in per_axis]
        n += 1
    assert n > 8


def test_signal_keys_against_numpy():
    sy, sx = 12, 10
    rows, cols = np.arange(sy), np.arange(sx)
    keys = [slice(None), slice(1, None), slice(None, -1), slice(5, 55), slice(-3, None), slice(0, None, 2), slice(1, 9, 3),
            slice(4, 5)]
    for kx in keys:
        for ky in keys:
            (r0, rs, nr), (c0, cs, nc) = _selection.signal_selection((sy, sx), (kx, ky))
            assert np.array_equal(np.arange(r0, r0 + rs * nr, rs)[:nr], rows[ky]) and nr == len(rows[ky])
            assert np.array_equal(np.arange(c0, c0 + cs * nc, cs)[:nc], cols[kx]) and nc == len(cols[kx])
    (r0, rs, nr), (c0, cs, nc) = _selection.signal_selection((sy, sx), slice(2, 4))  # one key: x, that is columns
    assert (r0, rs, nr, c0, cs, nc) == (0, 1, sy, 2, 1, 2)


def test_refused_keys():
    with pytest.raises(ValueError, match="would remove a signal axis"):
        _selection.signal_selection((12, 10), (3, slice(None)))
    for key in [1.5, (slice(0.5, 3), 0), np.float64(2), slice(0, 4, 1.0), True, "x", [0, 1], None]:
        with pytest.raises(TypeError):
            _selection.navigation_selection((7, 9), key)
    for key in [slice(None, None, -1), slice(5, 1, -2), slice(None, None, 0)]:
        with pytest.raises(ValueError, match="step must be positive"):
            _selection.navigation_selection((7, 9), key)
        with pytest.raises(ValueError, match="step must be positive"):
            _selection.signal_selection((12, 10), key)
    for key in [9, -10, (0, 7), (0, 0, 0)]:
        with pytest.raises(IndexError):
            _selection.navigation_selection((7, 9), key)
    with pytest.raises(IndexError, match="selects nothing"):
        _selection.signal_selection((12, 10), slice(5, 5))
    with pytest.raises(IndexError, match="no navigation axes"):
        _selection.navigation_selection((), 0)


def test_crop_axes():
    assert [_selection.crop_axis(a, 2) for a in (0, 1, 2, 3, "x", "y", "dx", "dy", -1)] == [
        ("navigation", 0), ("navigation", 1), ("signal", 0), ("signal", 1), ("navigation", 0), ("navigation", 1),
        ("signal", 0), ("signal", 1), ("signal", 1)]
    assert [_selection.crop_axis(a, 1) for a in (0, 1, 2, "x", "dx", "dy")] == [
        ("navigation", 0), ("signal", 0), ("signal", 1), ("navigation", 0), ("signal", 0), ("signal", 1)]
    assert _selection.crop_axis(0, 0) == ("signal", 0)
    for bad in (4, -5, "y ", "z"):
        with pytest.raises(ValueError):
            _selection.crop_axis(bad, 2)
    with pytest.raises(ValueError):
        _selection.crop_axis("y", 1)
    with pytest.raises(TypeError):
        _selection.crop_axis(1.0, 2)


# ---------------------------------------------------------------- select_plan.h
PLAN_PROBE = r"""
#include <cstdio>
#include "select_plan.h"
using namespace kpdi;
int main() {
  long long v[10];
  while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8,
               v + 9) == 10) {
    const SelPlan p = select_plan((int)v[0], (int)v[1], (int)v[2], v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8],
                                  (int)v[9]);
    printf("%d %u %u %u %u %u %u %u\n", p.path, p.run_bytes, p.runs, p.out_bytes, p.items, p.patterns_per_block, p.grid_x,
           p.grid_y);
  }
  return 0;
}
"""


def test_path_choice(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    asked = []
    for dtype in cases.DTYPES:
        es = np.dtype(dtype).itemsize
        for sy, sx in cases.DETECTORS:
            for n in cases.COUNTS:
                for name, rows, cols in cases.rectangles(sy, sx):
                    for _, idx in cases.index_lists(n):
                        asked.append((es, sy, sx, n if idx is None else len(idx)) + tuple(rows) + tuple(cols))
    # beyond the table: a tutorial-sized map, a large detector, and arguments that are no selection
    asked += [(1, 60, 60, 4125, 0, 1, 60, 0, 1, 60), (1, 60, 60, 4125, 10, 1, 40, 5, 1, 50), (4, 480, 480, 300, 0, 1, 480, 0, 1, 480),
              (2, 2048, 2048, 70000, 0, 2, 1024, 3, 1, 2000), (8, 480, 480, 3, 0, 1, 480, 0, 5, 96)]
    bad = [(3, 5, 7, 1, 0, 1, 5, 0, 1, 7), (1, 5, 7, 0, 0, 1, 5, 0, 1, 7), (1, 5, 7, 1, 0, 0, 5, 0, 1, 7),
           (1, 5, 7, 1, 0, 1, 6, 0, 1, 7), (1, 5, 7, 1, 0, 1, 5, 1, 1, 7), (1, 5, 7, 1, 2, 2, 3, 0, 1, 7),
           (1, 5, 7, 1, -1, 1, 2, 0, 1, 7), (1, 5, 7, 1, 0, 1, 5, 0, 3, 4), (1, 5, 7, 1, 0, 1, 0, 0, 1, 7),
           (8, 16384, 16384, 1, 0, 1, 1, 0, 1, 1)]
    text = "".join(" ".join(str(v) for v in a) + "\n" for a in asked + bad)
    lines = subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert len(lines) == len(asked) + len(bad)
    assert all(line.split()[0] == "-1" for line in lines[len(asked):])
    seen = set()
    for a, line in zip(asked, lines):
        es, sy, sx, n, r0, rs, nr, c0, cs, nc = a
        path, run_bytes, runs, out_bytes, items, ppb, gx, gy = map(int, line.split())
        # the path follows from how long the contiguous runs of wanted source bytes are
        if cs > 1 and nc > 1:
            want = 2
        elif nc == sx and (rs == 1 or nr == 1):
            want = 0
        else:
            want = 1
        assert path == want, a
        assert out_bytes == nr * nc * es
        if path == 2:
            assert items == nr * nc
        else:
            assert runs == (1 if path == 0 else nr) and run_bytes * runs == out_bytes
            # enough 16-byte pieces for an output pattern that starts at any byte, and no more than one to spare
            assert items * 16 >= out_bytes + 15 and (items - 1) * 16 < out_bytes + 15
        # every item of every pattern has a lane; the grid is sized from the work
        assert 1 <= ppb <= 64 and (ppb == 1 or ppb * items <= 256) and gx * 256 >= (items if ppb == 1 else 1)
        assert (gx - 1) * 256 < items
        groups = -(-n // ppb)
        assert gy == min(groups, 65535)
        seen.add(path)
        if n >= 65:
            assert gx * gy >= 2, a  # 65 is the first count that spans two workgroups whatever the shape
    assert seen == {0, 1, 2}


# ---------------------------------------------------------------- signatures
def params(fn):
    return [(n, p.default) for n, p in inspect.signature(fn).parameters.items() if n != "self"]


def test_signatures():
    """The reference's parameters (signals/ebsd.py:267-269, hyperspy's crop / crop_signal, detectors/_ebsd_detector.py:986,
    signals/util/array_tools.py:21-25), hard-coded."""
    E = inspect.Parameter.empty
    assert params(kpa.EBSD.extract_grid) == [("grid_shape", E), ("return_indices", False)]
    assert params(kpa.EBSD.crop) == [("axis", E), ("start", None), ("end", None), ("convert_units", False)]
    assert params(kpa.EBSD.crop_signal) == [("top", None), ("bottom", None), ("left", None), ("right", None),
                                            ("convert_units", False)]
    assert params(EBSDDetector.crop) == [("extent", E)]
    assert params(_selection.grid_indices) == [("grid_shape", E), ("nav_shape", E), ("return_spacing", False)]
    assert params(kpa.EBSD.to_device) == [] and params(kpa.EBSD.to_host) == []
    for name in ("inav", "isig", "is_resident", "data"):
        assert isinstance(getattr(kpa.EBSD, name), property), name
    assert kpa.EBSD.data.fset is not None


# ---------------------------------------------------------------- host-backed signals
def signal(nav=(7, 9), sig=(12, 10), dtype=np.uint8, per_point_pc=True):
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, nav + sig).astype(dtype)
    pc = np.array([0.42, 0.78, 0.5]) + 0.02 * rng.random(nav + (3,)) if per_point_pc else (0.42, 0.78, 0.5)
    s = kpa.EBSD(data, static_background=rng.integers(1, 256, sig).astype(dtype),
                 detector=EBSDDetector(shape=sig, pc=pc, sample_tilt=69.5, tilt=5.0), step_sizes=(1.5, 2.0)[:len(nav)])
    return s, data


class IndexableXmap:
    """A crystal map that can be indexed: its `shape` follows."""

    def __init__(self, ids):
        self.ids = np.asarray(ids)

    shape = property(lambda self: self.ids.shape)

    def __getitem__(self, key):
        if isinstance(key, np.ndarray) and key.dtype == bool and key.ndim == 1:  # (orix: a mask over the flattened map)
            return IndexableXmap(self.ids.ravel()[key])
        return IndexableXmap(self.ids[key])

    def deepcopy(self):
        return IndexableXmap(self.ids.copy())


def test_isig_crop_and_crop_signal_agree():
    """examples/selecting_data/crop_signal_axes.py: isig[5:55, 10:50] = crop(2, 5, 55) + crop("dy", 10, 50) =
    crop_signal(top=10, bottom=50, left=5, right=55); here on 12 x 10 patterns."""
    s, data = signal()
    bg, det = s.static_background.copy(), s.detector.deepcopy()
    s2 = s.isig[2:9, 1:11]
    assert not s2.is_resident and s2.data.flags.c_contiguous and not np.shares_memory(s2.data, data)
    assert np.array_equal(s2.data, data[:, :, 1:11, 2:9])
    assert np.array_equal(s2.static_background, bg[1:11, 2:9]) and s2.static_background.flags.c_contiguous
    want = det.crop((1, 11, 2, 9))
    assert s2.detector.shape == (10, 7) and np.array_equal(s2.detector.pc, want.pc)
    assert s2.step_sizes == s.step_sizes
    # the source is untouched
    assert np.array_equal(s.data, data) and np.array_equal(s.static_background, bg) and s.detector.shape == (12, 10)
    s3 = s.deepcopy()
    assert s3.crop(2, start=2, end=9) is None and s3.crop("dy", start=1, end=11) is None
    s4 = s.deepcopy()
    assert s4.crop_signal(top=1, bottom=11, left=2, right=9) is None
    for other in (s3, s4):
        assert np.array_equal(other.data, s2.data) and np.array_equal(other.static_background, s2.static_background)
        assert other.detector.shape == (10, 7) and np.allclose(other.detector.pc, s2.detector.pc, rtol=0, atol=1e-15)
    # steps: the detector cannot be cropped and gets the default PC
    s5 = s.isig[::2, 1::3]
    assert np.array_equal(s5.data, data[:, :, 1::3, ::2]) and np.array_equal(s5.static_background, bg[1::3, ::2])
    assert s5.detector.shape == (4, 5) and s5.detector.navigation_shape == (1,)
    assert s5.detector.pc.tolist() == [[0.5, 0.5, 0.5]] and s5.detector.sample_tilt == 69.5 and s5.detector.tilt == 5.0


def test_inav_and_crop_of_navigation_axes():
    """examples/selecting_data/crop_navigation_axes.py: inav[:, 0] is the first map row with one navigation axis;
    crop(1, 0, 1) leaves it as a row of a 2-D map."""
    s, data = signal()
    s.xmap = IndexableXmap(np.arange(63).reshape(7, 9))
    pcs = s.detector.pc.copy()
    s2 = s.inav[:, 0]
    assert np.array_equal(s2.data, data[0]) and s2.data.flags.c_contiguous and not np.shares_memory(s2.data, data)
    assert s2.xmap.shape == (9,) and np.array_equal(s2.xmap.ids, np.arange(9))
    assert s2.detector.navigation_shape == (9,) and np.array_equal(s2.detector.pc, pcs[0])
    assert s2.step_sizes == (2.0,) and np.array_equal(s2.static_background, s.static_background)
    s3 = s.deepcopy()
    s3.xmap = IndexableXmap(np.arange(63).reshape(7, 9))
    s3.crop(1, start=0, end=1)
    assert s3.data.shape == (1, 9, 12, 10) and np.array_equal(s3.data[0], s2.data)
    assert s3.xmap.shape == (1, 9) and s3.detector.navigation_shape == (1, 9) and s3.step_sizes == (1.5, 2.0)
    # ints, negative indices, steps: as NumPy reads them, in (x, y) order
    s4 = s.inav[1::2, -3:]
    assert np.array_equal(s4.data, data[-3:, 1::2]) and np.array_equal(s4.detector.pc, pcs[-3:, 1::2])
    assert s4.step_sizes == (1.5, 4.0) and np.array_equal(s4.xmap.ids, np.arange(63).reshape(7, 9)[-3:, 1::2])
    s5 = s.inav[-1, 2]
    assert np.array_equal(s5.data, data[2, -1]) and s5.data.shape == (12, 10) and s5.step_sizes == ()
    assert s5.detector.navigation_shape == (1,) and np.array_equal(s5.detector.pc[0], pcs[2, -1])
    assert np.array_equal(s.inav[4].data, data[:, 4])
    # an xmap that cannot be indexed is dropped, one PC stays
    t, tdata = signal(per_point_pc=False)
    t._xmap = kpa.signals.DictionaryXmap.empty((7, 9))
    t2 = t.inav[2:4, 1:3]
    assert t2.xmap is None and t2.detector.navigation_shape == (1,) and np.array_equal(t2.data, tdata[1:3, 2:4])
    # 1-D maps
    u, udata = signal(nav=(9,))
    assert np.array_equal(u.inav[2:7:2].data, udata[2:7:2]) and u.inav[3].data.shape == (12, 10)
    u.crop("x", 1, 4)
    assert np.array_equal(u.data, udata[1:4]) and u.detector.navigation_shape == (3,)


def test_selection_refusals_on_a_signal():
    s, data = signal()
    for bad, exc in [(lambda: s.isig[3], ValueError), (lambda: s.isig[:, 3], ValueError), (lambda: s.inav[1.5], TypeError),
                     (lambda: s.isig[0.2:0.8], TypeError), (lambda: s.inav[::-1], ValueError),
                     (lambda: s.isig[::-1, :], ValueError), (lambda: s.inav[0, 0, 0], IndexError),
                     (lambda: s.inav[9], IndexError), (lambda: s.crop(0, 1.0, 3), TypeError),
                     (lambda: s.crop(4), ValueError), (lambda: s.crop("z"), ValueError),
                     (lambda: s.crop(0, 1, 3, convert_units=True), NotImplementedError),
                     (lambda: s.crop_signal(top=1, convert_units=True), NotImplementedError),
                     (lambda: s.crop(0, 5, 5), IndexError)]:
        with pytest.raises(exc):
            bad()
    assert np.array_equal(s.data, data) and s.detector.shape == (12, 10)
    with pytest.raises(IndexError):
        kpa.EBSD(data[0, 0]).inav[0]


def test_extract_grid():
    s, data = signal()
    s.xmap = IndexableXmap(np.arange(63).reshape(7, 9))
    pcs = s.detector.pc.copy()
    for grid in [(3, 2), (2, 3), (1, 1), (8, 6)]:
        want = _selection.grid_indices(grid[::-1], (7, 9))
        s2, idx = s.extract_grid(grid, return_indices=True)
        assert np.array_equal(idx, want)
        assert np.array_equal(s2.data, data[tuple(idx)]) and s2.data.shape == idx.shape[1:] + (12, 10)
        assert np.array_equal(s2.detector.pc, pcs[tuple(idx)])
        assert np.array_equal(np.sort(s2.xmap.ids.ravel()), np.sort((idx[0] * 9 + idx[1]).ravel()))
        spacing = np.ceil(np.array((7, 9)) / (np.array(grid[::-1]) + 1)).astype(int)
        assert s2.step_sizes == (1.5 * spacing[0], 2.0 * spacing[1])
        assert np.array_equal(s2.static_background, s.static_background)
        assert not np.shares_memory(s2.static_background, s.static_background)
    assert np.array_equal(s.extract_grid((3, 2)).data, data[tuple(_selection.grid_indices((2, 3), (7, 9)))])
    # the reference's error text, shapes in HyperSpy's order
    with pytest.raises(ValueError, match=r"grid_shape \(10, 2\) must be compatible with navigation shape \(9, 7\)"):
        s.extract_grid((10, 2))
    with pytest.raises(ValueError, match=r"grid_shape \(3,\) must be compatible with navigation shape \(9, 7\)"):
        s.extract_grid(3)
    # 1-D map; a detector whose PCs do not belong to the map gets the default
    u, udata = signal(nav=(9,), per_point_pc=False)
    u2, idx = u.extract_grid(3, return_indices=True)
    assert idx.tolist() == [[3, 6]] and np.array_equal(u2.data, udata[idx[0]]) and u2.detector.navigation_shape == (1,)
    assert u2.step_sizes == (1.5 * 3,)


def test_host_backed_is_the_default_and_data_is_assignable():
    s, data = signal()
    assert not s.is_resident and s.data is data and s.to_host() is s
    other = data[:2].copy()
    s.data = other
    assert s.data is other and s._navigation_shape_rc == (2, 9) and not s.is_resident
