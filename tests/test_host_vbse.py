"""Virtual BSE imaging without a GPU: the ROI -> pixel rule, the grid of `VirtualBSEImager`, its errors, the channel
arithmetic of `get_rgb_image` against the reference's fixture (tests/golden/vbse.npz, made by the reference's own
`_get_rgb_image`, tools/gen_vbse_golden.py) with the sums taken from the NumPy restatement (tests/_vbse_restate.py),
the reference's known answers, how the new callables bind, and the plan of csrc/regionsum_plan.h compiled with the host
compiler."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import _vbse_cases as cases
import _vbse_restate as R
import kikuchipy_amd as kpa
from conftest import GOLDEN, ROOT
from kikuchipy_amd import imaging
from kikuchipy_amd.imaging import RectangularROI, VirtualBSEImager, roi_to_rect

FIX = np.load(os.path.join(GOLDEN, "vbse.npz"))

# the reference's parameters, in its order, with its literal defaults (imaging/vbse.py, signals/ebsd.py:1555-1559,
# signals/virtual_bse_image.py); what this package adds is keyword-only
SIGNATURES = {
    "imaging.VirtualBSEImager": (["signal"], {}),
    "imaging.VirtualBSEImager.get_rgb_image": (
        ["self", "r", "g", "b", "percentiles", "normalize", "alpha", "dtype_out", "add_bright", "contrast"],
        {"percentiles": None, "normalize": True, "alpha": None, "dtype_out": "uint8", "add_bright": 0, "contrast": 1.0}),
    "imaging.VirtualBSEImager.get_images_from_grid": (["self", "dtype_out"], {"dtype_out": "float32"}),
    "imaging.VirtualBSEImager.roi_from_grid": (["self", "index"], {}),
    "imaging.RectangularROI": (["left", "top", "right", "bottom"], {"left": None, "top": None, "right": None, "bottom": None}),
    "EBSD.get_virtual_bse_intensity": (["self", "roi", "out_signal_axes"], {"out_signal_axes": None}),
    "VirtualBSEImage.rescale_intensity": (
        ["self", "relative", "in_range", "out_range", "dtype_out", "percentiles", "show_progressbar", "inplace", "lazy_output"],
        {"relative": False, "in_range": None, "out_range": None, "dtype_out": None, "percentiles": None,
         "show_progressbar": None, "inplace": True, "lazy_output": None}),
    "VirtualBSEImage.normalize_intensity": (
        ["self", "num_std", "divide_by_square_root", "dtype_out", "show_progressbar", "inplace", "lazy_output"],
        {"num_std": 1, "divide_by_square_root": False, "dtype_out": None, "show_progressbar": None, "inplace": True,
         "lazy_output": None}),
    "VirtualBSEImage.adaptive_histogram_equalization": (
        ["self", "kernel_size", "clip_limit", "nbins", "show_progressbar", "inplace", "lazy_output"],
        {"kernel_size": None, "clip_limit": 0.0, "nbins": 128, "show_progressbar": None, "inplace": True,
         "lazy_output": None}),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_reference_calls_bind_the_same_way(name):
    obj = kpa
    for part in name.split("."):
        obj = getattr(obj, part)
    positional, defaults = SIGNATURES[name]
    params = list(inspect.signature(obj).parameters.values())
    assert [p.name for p in params if p.kind == p.POSITIONAL_OR_KEYWORD] == positional
    for p in params:
        if p.name in defaults:
            assert p.default == defaults[p.name] and type(p.default) is type(defaults[p.name]), (name, p.name)
        elif p.name not in positional:
            assert p.kind == p.KEYWORD_ONLY and p.default is not p.empty, (name, p.name)


def test_package_exports():
    assert kpa.imaging is imaging and "imaging" in kpa.__all__ and "VirtualBSEImage" in kpa.__all__
    from kikuchipy_amd import pattern, signals

    assert signals.VirtualBSEImage is kpa.VirtualBSEImage and callable(pattern.region_sums)


# ---- the ROI rule
def test_roi_rule_whole_pixels_and_ends():
    assert roi_to_rect(RectangularROI(0, 0, 10, 10), (60, 60)) == (0, 10, 0, 10)
    assert roi_to_rect(RectangularROI(left=12, top=24, right=60, bottom=36), (60, 60)) == (24, 36, 12, 60)
    assert roi_to_rect(RectangularROI(), (24, 20)) == (0, 24, 0, 20)
    assert roi_to_rect(RectangularROI(-3, -0.6, 100, 59.2), (60, 60)) == (0, 60, 0, 60)  # 59.2 lies beyond pixel 59
    assert roi_to_rect(RectangularROI(70, 5, 80, 3), (60, 60)) == (5, 5, 60, 60)  # empty, never reversed


def test_roi_rule_rounds_half_to_even_and_uses_the_axes():
    assert roi_to_rect(RectangularROI(7.5, 22.5, 37.5, 52.5), (60, 60)) == (22, 52, 8, 38)
    assert roi_to_rect(RectangularROI(0.5, 1.5, 2.5, 3.5), (60, 60)) == (2, 4, 0, 2)
    # scale 0.5 and offset 10 along x, scale 2 along y
    assert roi_to_rect(RectangularROI(left=11, top=4, right=20, bottom=9), (60, 60), ((0.5, 10.0), (2.0, 0.0))) == (2, 4, 2, 20)


def test_roi_rule_is_the_restatement_over_a_sweep():
    rng = np.random.default_rng(0)
    for shape in ((60, 60), (24, 20), (3, 3)):
        for _ in range(300):
            v = np.round(rng.uniform(-5, max(shape) + 5, 4) * 4) / 4  # quarters: many exact halves
            roi = RectangularROI(*v)
            assert roi_to_rect(roi, shape) == R.roi_rect(*v, shape)


def test_other_roi_kinds_and_hyperspy_like_objects():
    class CircleROI:
        cx = cy = r = 5

    with pytest.raises(NotImplementedError, match="CircleROI"):
        roi_to_rect(CircleROI(), (60, 60))

    class Theirs:  # anything with the four attributes
        left, top, right, bottom = 1.0, 2.0, 5.0, 7.0

    assert roi_to_rect(Theirs(), (60, 60)) == (2, 7, 1, 5)

    class Axis:
        def __init__(self, scale, offset):
            self.scale, self.offset = scale, offset

    class Signal:
        class axes_manager:
            signal_axes = [Axis(0.5, 10.0), Axis(2.0, 0.0)]

    assert imaging.signal_axes(Signal()) == ((0.5, 10.0), (2.0, 0.0))
    assert imaging.signal_axes(kpa.EBSD(np.zeros((2, 3, 3), np.uint8))) == ((1.0, 0.0), (1.0, 0.0))


# ---- the imager
def test_init_repr_and_default_grid():
    s = kpa.EBSD(cases.inputs("dummy"))
    imager = VirtualBSEImager(s)
    assert imager.signal is s and imager.grid_shape == (3, 3)
    assert repr(imager) == "VirtualBSEImager for " + repr(s)
    assert VirtualBSEImager(kpa.EBSD(cases.inputs("ni"))).grid_shape == (5, 5)
    assert VirtualBSEImager(kpa.EBSD(np.zeros((4, 60), np.uint8))).grid_shape == (4, 5)


@pytest.mark.parametrize("grid", [(10, 10), (13, 7)])
def test_set_grid_shape(grid):
    imager = VirtualBSEImager(kpa.EBSD(cases.inputs("ni")))
    imager.grid_shape = grid
    assert imager.grid_shape == grid
    assert imager.grid_rows.dtype == np.float64 and np.array_equal(imager.grid_rows, np.linspace(0, 60, grid[0] + 1))
    assert np.array_equal(imager.grid_cols, np.linspace(0, 60, grid[1] + 1))


def test_grid_shape_errors():
    imager = VirtualBSEImager(kpa.EBSD(cases.inputs("ni")))
    with pytest.raises(ValueError, match="Grid shape must have the same length as number of signal dimensions 2"):
        imager.grid_shape = (5,)
    with pytest.raises(ValueError, match=r"Grid shape \(n rows, n cols\) = \(61, 5\) cannot be greater than signal shape \(60, 60\)"):
        imager.grid_shape = (61, 5)
    assert imager.grid_shape == (5, 5)


def test_roi_from_grid_is_the_restatement():
    imager = VirtualBSEImager(kpa.EBSD(np.zeros((1, 60, 60), np.uint8)))
    for grid in ((5, 5), (8, 8), (13, 7), (60, 60), (1, 1)):
        imager.grid_shape = grid
        for idx in list(np.ndindex(*grid))[:: max(1, grid[0] * grid[1] // 40)]:
            roi = imager.roi_from_grid(idx)
            assert (roi.left, roi.top, roi.right, roi.bottom) == R.tile_roi((60, 60), grid, idx)
            assert imager._rect(idx) == R.tile_rect((60, 60), grid, idx)
    imager.grid_shape = (5, 5)
    roi = imager.roi_from_grid([(0, 1), (0, 2)])
    assert (roi.left, roi.top, roi.right, roi.bottom) == (12, 0, 36, 12)
    # (8, 8): edges at x.5 go to the even pixel; the tiles still cover the detector once
    cover = np.zeros((60, 60), int)
    for r0, r1, c0, c1 in R.grid_rects((60, 60), (8, 8)):
        cover[r0:r1, c0:c1] += 1
    assert R.tile_rect((60, 60), (8, 8), (0, 0)) == (0, 8, 0, 8) and R.tile_rect((60, 60), (8, 8), (3, 2)) == (22, 30, 15, 22)
    assert np.all(cover == 1)


def test_rgb_errors_before_any_gpu_work():
    one_d = VirtualBSEImager(kpa.EBSD(cases.inputs("ni")[0]))
    with pytest.raises(ValueError, match="The signal dimension cannot be "):
        one_d.get_rgb_image(r=(0, 0), g=(0, 1), b=(0, 2))
    imager = VirtualBSEImager(kpa.EBSD(cases.inputs("ni")))
    with pytest.raises(ValueError, match="dtype_out must be uint8 or uint16"):
        imager.get_rgb_image(r=(0, 0), g=(0, 1), b=(0, 2), dtype_out=np.float32)
    with pytest.raises(ValueError, match="The length of 'out_signal_axes' cannot be longer"):
        imager.signal.get_virtual_bse_intensity(RectangularROI(0, 0, 5, 5), out_signal_axes=[0, 1, 2])


# ---- the channel arithmetic against the reference
@pytest.mark.parametrize("name", list(cases.RGB_CASES))
def test_rgb_arithmetic_is_the_reference(name):
    inp, grid, r, g, b, kw = cases.RGB_CASES[name]
    data = cases.inputs(inp)
    kw = dict(kw, alpha=cases.alpha(kw.get("alpha")))
    chans = R.channels(data, grid, r, g, b)
    got = imaging.rgb_image(chans, **kw)
    want = FIX[cases.rgb_key(name)]
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(R.rgb(chans, **kw), want)
    if name in cases.KNOWN_RGB_MEAN:
        assert cases.close_to_known(got.mean(), *cases.KNOWN_RGB_MEAN[name])
        assert float(FIX["known__" + name]) == cases.KNOWN_RGB_MEAN[name][0]


def test_restated_grid_images_are_the_fixture():
    for inp, grid, dtype_out in cases.GRID_CASES:
        want = FIX[cases.grid_key(inp, grid, dtype_out)]
        got = R.images_from_grid(cases.inputs(inp), grid, dtype_out)
        if cases.inputs(inp).dtype.kind in "iu" or np.dtype(dtype_out).kind == "f":
            assert got.dtype == want.dtype and np.array_equal(got, want), (inp, grid, dtype_out)
    assert np.allclose(FIX[cases.grid_key("dummy", (1, 1), "float32")].mean(), cases.KNOWN_DUMMY_1X1_MEAN)


def test_virtual_bse_image_object():
    rgb = FIX[cases.rgb_key("ni_default")]
    image = kpa.VirtualBSEImage(rgb)
    assert image.rgb_data.dtype == np.dtype([("R", "u1"), ("G", "u1"), ("B", "u1")]) and image.rgb_data.shape == (3, 3)
    assert np.array_equal(image.rgb_data["G"], rgb[..., 1])
    u16 = kpa.VirtualBSEImage(FIX[cases.rgb_key("ni_u16")])
    assert u16.rgb_data.dtype == np.dtype([("R", "u2"), ("G", "u2"), ("B", "u2")])
    copy = image.deepcopy()
    copy.data[0, 0, 0] += 1
    assert image.data[0, 0, 0] == rgb[0, 0, 0]
    with pytest.raises(ValueError, match="not an RGB image"):
        kpa.VirtualBSEImage(np.zeros((3, 3), np.float32)).rgb_data
    with pytest.raises(ValueError, match="'lazy_output=True' requires 'inplace=False'"):
        image.rescale_intensity(lazy_output=True)
    with pytest.raises(ValueError, match="'percentiles' must be None if 'in_range' is not None"):
        image.rescale_intensity(in_range=(0, 1), percentiles=(1, 99))


def test_region_sums_checks_its_rectangles_on_the_host():
    from kikuchipy_amd.pattern import region_sums

    data = np.zeros((2, 6, 5), np.uint8)
    for bad in ([(0, 7, 0, 5)], [(0, 6, 0, 6)], [(3, 2, 0, 5)], [(0, 6, 4, 3)], [(-1, 2, 0, 5)]):
        with pytest.raises(ValueError, match="not inside the 6 x 5 detector"):
            region_sums(data, bad)
    with pytest.raises(ValueError, match="rects must be integers of shape"):
        region_sums(data, [(0, 1, 2)])
    with pytest.raises(ValueError, match="rects must be integers of shape"):
        region_sums(data, [(0.0, 1.0, 2.0, 3.0)])


# ---- the plan
PLAN_PROBE = r"""
#include <cstdio>
#include <initializer_list>
#include "regionsum_plan.h"
int main() {
  const int shapes[][2] = {{60, 60}, {240, 240}, {24, 20}, {1001, 1001}, {1024, 1024}, {3, 3}, {1, 5000}, {60, 9000}};
  const int dtypes[] = {KPDI_U8, KPDI_I16, KPDI_F32, KPDI_F64};
  for (auto &s : shapes)
    for (int d : dtypes)
      for (int nr : {1, 25, 5000}) {
        kpdi::RsPlan p = kpdi::rs_plan(d, s[0], s[1], 1000, nr);
        printf("%d %d %d %d %d %d %d %zu %zu %lld %zu\n", s[0], s[1], kpdi::pattern_dtype_bytes(d), nr, p.path, p.rows_per_block,
               p.blocks_per_pattern, p.slot_bytes, p.lds_bytes, (long long)p.batch, p.workspace_bytes);
      }
}
"""


@pytest.mark.skipif(not shutil.which("g++"), reason="needs a host C++ compiler")
def test_plan_bounds(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text(PLAN_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    rows = [[int(v) for v in line.split()] for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                                        text=True).stdout.splitlines()]
    assert len(rows) == 8 * 4 * 3
    for sy, sx, es, nr, path, rb, nblk, slot, lds, batch, ws in rows:
        if sx * es > 8192:  # a row does not fit a wave's block
            assert path == -1
            continue
        assert path == (0 if nblk == 1 else 1), (sy, sx, es)
        assert 1 <= rb <= sy and rb * sx * es <= 8192 and nblk == -(-sy // rb)
        assert (rb + 1) * sx * es > 8192 or rb == sy  # as many rows as fit
        assert slot % 16 == 0 and slot >= rb * sx * es + 30  # an unaligned block: up to 15 bytes before, 15 after
        assert lds == 256 * 16 + 4 * slot and lds <= 150 * 1024
        if path == 1:
            assert 1 <= batch <= 1000 and ws == batch * nblk * nr * 8 and ws <= 256 << 20
    by = {(r[0], r[1], r[2], r[3]): r for r in rows}
    assert by[(60, 60, 1, 25)][4:7] == [0, 60, 1]      # a 60 x 60 uint8 pattern is one block: four patterns per workgroup
    assert by[(240, 240, 1, 25)][4:7] == [1, 34, 8]
    assert by[(1024, 1024, 8, 25)][4:7] == [1, 1, 1024]
    assert by[(1024, 1024, 8, 5000)][9] < 1000          # batches once the partial sums pass the workspace cap
