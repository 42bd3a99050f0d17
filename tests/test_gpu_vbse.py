"""Virtual BSE imaging on the GPU (csrc/regionsum.hip through kpdi_region_sums): region sums, `EBSD.get_virtual_bse_intensity`
and `VirtualBSEImager` against the reference's fixture (tests/golden/vbse.npz) and the NumPy restatement
(tests/_vbse_restate.py) for the shapes the fixture does not hold.

Integer patterns: everything exact.  Float patterns: |gpu - restatement| <= n 2^-24 sum|x| per region (float32; 2^-52 for
float64), n the region's pixels and sum|x| from the restatement in float64: any order of summing n float32 terms is within
(n - 1) 2^-24 sum|x| of the exact sum, and the GPU's float64 accumulation rounds once.  RGB images of float patterns are
compared through the channel sums (the bound above) and, given the GPU's own sums, exactly through the host arithmetic:
a per-pixel "within one grey level where the bound reaches an integer" test would need the bound propagated through
median, std and percentiles."""

import json
import os

import numpy as np
import pytest

import _vbse_cases as cases
import _vbse_restate as R
import kikuchipy_amd as kpa
from conftest import GOLDEN
from kikuchipy_amd import _lib
from kikuchipy_amd.imaging import RectangularROI, VirtualBSEImager, rgb_image
from kikuchipy_amd.pattern import region_sums

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(GOLDEN, "vbse.npz"))
INT_DTYPES = [np.uint8, np.int8, np.uint16, np.int16]
EPS = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -52}


def make(shape, dtype, seed=0, n=5):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return rng.integers(info.min, int(info.max) + 1, (n,) + tuple(shape)).astype(dt)
    return ((rng.random((n,) + tuple(shape)) - 0.3) * 1000).astype(dt)


def rect_list(shape, n, seed=1):
    """n rectangles: random ones (they overlap), some empty, the whole detector, single pixels."""
    rng = np.random.default_rng(seed)
    sy, sx = shape
    out = [(0, sy, 0, sx), (0, 0, 0, 0), (sy, sy, sx, sx), (sy - 1, sy, sx - 1, sx), (0, 1, 0, 1), (2, 2, 0, sx)]
    while len(out) < n:
        r = np.sort(rng.integers(0, sy + 1, 2))
        c = np.sort(rng.integers(0, sx + 1, 2))
        out.append((int(r[0]), int(r[1]), int(c[0]), int(c[1])))
    return out[:n]


def float_ratio(got, data, rects):
    """largest |got - restatement| / (n eps sum|x|) over the regions (0 where both are 0)."""
    s, a, n = R.region_sums_f64(data, rects)
    bound = n * EPS[data.dtype] * a
    err = np.abs(got.astype(np.float64) - s)
    assert np.all(err <= bound), float(np.max(err - bound))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))


@pytest.mark.parametrize("shape", [(60, 60), (240, 240), (24, 20)])
@pytest.mark.parametrize("dtype", INT_DTYPES)
@pytest.mark.parametrize("n_rects", [1, 25, 210])
def test_integer_region_sums_are_exact(shape, dtype, n_rects):
    data = make(shape, dtype)
    rects = rect_list(shape, n_rects) if n_rects != 25 else R.grid_rects(shape, (5, 5))
    got = region_sums(data, rects)
    want = R.region_sums(data, rects)
    assert got.dtype == want.dtype and got.dtype == (np.uint64 if np.dtype(dtype).kind == "u" else np.int64)
    assert got.shape == (len(data), n_rects)
    assert np.array_equal(got, want)


def test_float_region_sums_within_the_summation_bound():
    worst = {}
    for shape, n in (((60, 60), 5), ((240, 240), 3), ((24, 20), 5), ((1001, 1001), 1)):
        for dtype in (np.float32, np.float64):
            if shape == (1001, 1001) and dtype == np.float64:
                continue
            data = make(shape, dtype, n=n)
            for n_rects in (1, 25, 210):
                rects = rect_list(shape, n_rects) if n_rects != 25 else R.grid_rects(shape, (5, 5))
                got = region_sums(data, rects)
                assert got.dtype == dtype and got.shape == (n, n_rects)
                worst[f"{shape[0]}x{shape[1]}_{np.dtype(dtype).name}_{n_rects}"] = float_ratio(got, data, rects)
    out = os.environ.get("KPDI_VBSE_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"largest_error_over_bound": worst}, f, indent=1)
    print("largest |gpu - f64 restatement| / (n eps sum|x|):", max(worst.values()))


def test_large_detector_integer_1001_and_1024():
    for shape, dtype in (((1001, 1001), np.uint16), ((1024, 1024), np.uint8)):
        data = make(shape, dtype, n=2)
        rects = rect_list(shape, 30)
        assert np.array_equal(region_sums(data, rects), R.region_sums(data, rects))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
def test_special_values(dtype, shape):
    data = make(shape, dtype, n=4)
    sy, sx = shape
    h, w = sy // 2, sx // 2
    rects = [(0, h, 0, w), (0, h, w, sx), (h, sy, 0, w), (h, sy, w, sx), (0, sy, 0, sx)]
    clean = region_sums(data, rects)
    data[0, 1, 2] = np.nan            # counts as 0
    data[1, :h, :w] = np.nan          # a region of NaN only: 0
    data[2, 3, 3] = np.inf            # +inf
    data[3, 4, 4] = np.inf
    data[3, h - 1, w - 1] = -np.inf   # +inf and -inf in one region: NaN
    got = region_sums(data, rects)
    want = R.region_sums(data, rects)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert got[1, 0] == 0 and got[2, 0] == np.inf and got[2, 4] == np.inf and np.isnan(got[3, 0]) and np.isnan(got[3, 4])
    # the other regions of these patterns are not affected: the same bits as without the special values
    assert np.array_equal(got[:, 1:4], clean[:, 1:4])
    fin = np.isfinite(want)
    s, a, n = R.region_sums_f64(np.where(np.isfinite(data), data, 0), rects)
    assert np.all(np.abs(got.astype(np.float64) - s)[fin] <= (n * EPS[np.dtype(dtype)] * a)[fin])


@pytest.mark.parametrize("grid", [(1, 1), (5, 5), (13, 7), (8, 8), (60, 60)])
@pytest.mark.parametrize("dtype", [np.uint8, np.int16])
def test_grids_on_60x60(grid, dtype):
    """(8, 8) has tile edges at x.5: the rounding of the ROI rule (half to even) is exercised against the restatement, not
    against the reference, whose tests pin whole-pixel edges only."""
    data = make((60, 60), dtype, n=6).reshape(2, 3, 60, 60)
    imager = VirtualBSEImager(kpa.EBSD(data))
    imager.grid_shape = grid
    for dtype_out in ("float32", "float64", "uint16"):
        got = imager.get_images_from_grid(dtype_out).data
        want = R.images_from_grid(data, grid, dtype_out)
        assert got.dtype == want.dtype and got.shape == grid + (2, 3)
        assert np.array_equal(got, want)
    imager.signal.close()


def test_grid_images_of_the_fixture():
    for inp, grid, dtype_out in cases.GRID_CASES:
        data = cases.inputs(inp)
        imager = VirtualBSEImager(kpa.EBSD(data))
        imager.grid_shape = grid
        got = imager.get_images_from_grid(dtype_out).data
        want = FIX[cases.grid_key(inp, grid, dtype_out)]
        assert got.dtype == want.dtype and got.shape == want.shape, (inp, grid, dtype_out)
        if data.dtype.kind in "iu":
            assert np.array_equal(got, want), (inp, grid, dtype_out)
        elif np.dtype(dtype_out).kind == "f":
            # the fixture holds NumPy's pairwise float sums: both lie within the bound of the float64 restatement
            rects = R.grid_rects(data.shape[-2:], grid)
            s, a, n = R.region_sums_f64(data, rects)
            bound = np.moveaxis(n * EPS[data.dtype] * a, -1, 0).reshape(want.shape)
            centre = np.moveaxis(s, -1, 0).reshape(want.shape)
            # float64 sums stored as float32: the rounding of the output format on top
            cast = np.abs(centre) * 2.0 ** -24 if (data.dtype, np.dtype(dtype_out)) == (np.float64, np.float32) else 0
            assert np.all(np.abs(got - centre) <= bound + cast) and np.all(np.abs(want - centre) <= bound + cast)
        imager.signal.close()
    one = VirtualBSEImager(kpa.EBSD(cases.inputs("dummy")))
    assert one.grid_shape == (3, 3)
    one.grid_shape = (1, 1)
    assert np.allclose(one.get_images_from_grid().data.mean(), cases.KNOWN_DUMMY_1X1_MEAN)


def _channel(imager, spec):
    def one(roi):
        return RectangularROI(*roi[1:]) if len(roi) == 5 and roi[0] == "roi" else roi
    return one(spec) if isinstance(spec, tuple) else [one(v) for v in spec]


@pytest.mark.parametrize("name", list(cases.RGB_CASES))
def test_rgb_images_of_the_fixture(name):
    inp, grid, r, g, b, kw = cases.RGB_CASES[name]
    data = cases.inputs(inp)
    kw = dict(kw, alpha=cases.alpha(kw.get("alpha")))
    imager = VirtualBSEImager(kpa.EBSD(data))
    imager.grid_shape = grid
    image = imager.get_rgb_image(_channel(imager, r), _channel(imager, g), _channel(imager, b), **kw)
    want = FIX[cases.rgb_key(name)]
    assert isinstance(image, kpa.VirtualBSEImage) and image.data.dtype == want.dtype and image.data.shape == want.shape
    code = f"u{want.dtype.itemsize}"
    assert image.rgb_data.dtype == np.dtype([("R", code), ("G", code), ("B", code)]) and image.rgb_data.shape == want.shape[:2]
    if name in cases.INTEGER_RGB_CASES:
        assert np.array_equal(image.data, want), name
    else:
        # float patterns: through the channel sums (see the module docstring)
        shape = data.shape[-2:]
        rects = [q for ch in (r, g, b) for q in R.channel_rects(shape, grid, ch)]
        sums = region_sums(data, rects)
        float_ratio(sums, data, rects)
        chans, i = [], 0
        for ch in (r, g, b):
            chans.append(np.zeros(data.shape[:2], dtype=np.float64))
            for _ in R.channel_rects(shape, grid, ch):
                chans[-1] += sums[..., i]
                i += 1
        assert np.array_equal(image.data, rgb_image(chans, **kw))
    if name in cases.KNOWN_RGB_MEAN:
        assert cases.close_to_known(image.data.mean(), *cases.KNOWN_RGB_MEAN[name])
    imager.signal.close()


def test_rois_from_the_grid_give_the_tiles_and_alpha_as_an_image():
    s = kpa.EBSD(cases.inputs("ni"))
    imager = VirtualBSEImager(s)
    rois = [imager.roi_from_grid(i) for i in np.ndindex(imager.grid_shape)][:3]
    a = imager.get_rgb_image(r=rois[0], g=rois[1], b=rois[2])
    b = imager.get_rgb_image(r=(0, 0), g=(0, 1), b=(0, 2))
    assert np.array_equal(a.data, b.data)
    for r, g, bl in ([[(0, 1), (0, 2)], [(1, 1), (1, 2)], [(2, 1), (2, 2)]], [[(2, 1), (2, 2)], [(3, 1), (3, 2)], [(4, 1), (4, 2)]]):
        two = imager.get_rgb_image(r=r, g=g, b=bl)
        one = imager.get_rgb_image(r=imager.roi_from_grid(r), g=imager.roi_from_grid(g), b=imager.roi_from_grid(bl))
        assert np.array_equal(two.data, one.data)
    alpha = s.get_virtual_bse_intensity(roi=RectangularROI(0, 0, 10, 10))
    assert isinstance(alpha, kpa.VirtualBSEImage) and alpha.data.dtype == np.uint64
    assert np.array_equal(alpha.data, R.region_sum(s.data, (0, 10, 0, 10)))
    c = imager.get_rgb_image(r=(0, 1), g=(0, 2), b=(0, 3), alpha=alpha)
    d = imager.get_rgb_image(r=(0, 1), g=(0, 2), b=(0, 3), alpha=alpha.data)
    assert np.array_equal(c.data, d.data)
    with pytest.raises(ValueError, match="The signal dimension cannot be "):
        VirtualBSEImager(kpa.EBSD(cases.inputs("ni")[0])).get_rgb_image(r=(0, 0), g=(0, 1), b=(0, 2))
    s.close()


@pytest.mark.parametrize("dtype", INT_DTYPES + [np.float32])
@pytest.mark.parametrize("nav", [(), (5,), (2, 3)])
def test_get_virtual_bse_intensity(dtype, nav):
    data = make((60, 60), dtype, n=int(np.prod(nav)) if nav else 1).reshape(nav + (60, 60))
    keep = data.copy()
    s = kpa.EBSD(data)
    image = s.get_virtual_bse_intensity(RectangularROI(left=5, top=10, right=60, bottom=31.4))
    want = R.region_sum(keep, (10, 31, 5, 60))
    assert image.data.shape == nav and image.data.dtype == want.dtype
    if np.dtype(dtype).kind in "iu":
        assert np.array_equal(image.data, want)
    else:
        float_ratio(image.data[..., None], keep, [(10, 31, 5, 60)])
    assert np.array_equal(s.data, keep) and s.data is data
    if len(nav) == 2:
        t = s.get_virtual_bse_intensity(RectangularROI(5, 10, 60, 31.4), out_signal_axes=(1, 0))
        assert np.array_equal(t.data, image.data.T)
    with pytest.raises(ValueError, match="The length of 'out_signal_axes' cannot be longer"):
        s.get_virtual_bse_intensity(RectangularROI(0, 0, 5, 5), out_signal_axes=list(range(len(nav) + 1)))
    s.close()


@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
def test_resident_patterns_after_background_removal(shape):
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (4, 5) + shape).astype(np.uint8)
    bg = rng.integers(0, 40, shape).astype(np.uint8)
    rects = R.grid_rects(shape, (5, 5))
    with _lib.Context(0) as ctx:
        ctx.set_problem(*shape, None, _lib.METRIC_NCC, 1)
        ctx.set_experimental(p.reshape(-1, *shape))
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
        resident = ctx.region_sums(rects)  # the recorded steps run first
        corrected = ctx.get_experimental()
    assert np.array_equal(resident, R.region_sums(corrected, rects))
    s = kpa.EBSD(p.copy(), static_background=bg)
    s.remove_static_background()
    s.remove_dynamic_background()
    got = VirtualBSEImager(s).get_images_from_grid("float64").data
    assert np.array_equal(got, R.images_from_grid(s.data, (5, 5), "float64"))
    s.close()


@pytest.mark.parametrize("n_ctx", [2, 8])
@pytest.mark.parametrize("shape,dtype", [((60, 60), np.float32), ((240, 240), np.float32), ((60, 60), np.uint16)])
def test_block_wise_over_contexts(n_ctx, shape, dtype):
    data = make(shape, dtype, n=21).reshape((3, 7) + shape)
    rects = rect_list(shape, 40)
    one = region_sums(data, rects)
    ctxs = [_lib.Context(0) for _ in range(n_ctx)]
    try:
        many = region_sums(data, rects, contexts=ctxs)
    finally:
        for c in ctxs:
            c.close()
    assert many.shape == (3, 7, 40) and many.dtype == one.dtype
    assert np.array_equal(one, many)
    # ... nor on how many patterns are resident
    assert np.array_equal(region_sums(data[1, 2:4], rects), one[1, 2:4])


def test_image_methods_are_the_stack_functions():
    from kikuchipy_amd import pattern

    s = kpa.EBSD(make((24, 20), np.uint8, n=192).reshape(16, 12, 24, 20))
    imager = VirtualBSEImager(s)
    images = imager.get_images_from_grid("float32")
    assert images.data.shape == (5, 5, 16, 12)
    a = images.deepcopy()
    assert a.rescale_intensity(dtype_out=np.uint8) is None
    assert np.array_equal(a.data, pattern.rescale_intensity_stack(images.data, dtype_out=np.uint8))
    b = images.normalize_intensity(num_std=2, inplace=False)
    assert np.array_equal(b.data, pattern.normalize_intensity_stack(images.data, 2))
    c = a.adaptive_histogram_equalization(kernel_size=(4, 4), inplace=False)
    assert np.array_equal(c.data, pattern.adaptive_histogram_equalization_stack(a.data, (4, 4)))
    assert np.array_equal(images.data, imager.get_images_from_grid("float32").data)
    s.close()


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C

    EINVAL = -1  # KPDI_EINVAL of include/kpdi.h

    data = make((60, 60), np.uint8)
    for bad in ([(0, 61, 0, 5)], [(0, 5, 0, 61)], [(5, 4, 0, 5)], [(0, 5, 7, 6)], [(-1, 5, 0, 5)]):
        with pytest.raises(ValueError, match="not inside"):
            region_sums(data, bad)
    with _lib.Context(0) as ctx:
        ctx.set_problem(60, 60, None, _lib.METRIC_NCC, 1)
        ctx.set_experimental(data)
        f, h = _lib.load(), ctx._h
        out = np.zeros((5, 1), dtype=np.uint64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        for bad in ((0, 61, 0, 5), (0, 5, 0, 61), (5, 4, 0, 5), (0, 5, 7, 6), (-1, 5, 0, 5)):
            r = np.array([bad], dtype=np.int32)
            assert f.kpdi_region_sums(h, ptr(r), 1, ptr(out)) == EINVAL
            assert "not inside" in _lib.last_error()
        r = np.array([(0, 5, 0, 5)], dtype=np.int32)
        assert f.kpdi_region_sums(h, ptr(r), -1, ptr(out)) == EINVAL
        assert f.kpdi_region_sums(h, ptr(r), 1, None) == EINVAL
        assert f.kpdi_region_sums(h, None, 1, ptr(out)) == EINVAL
        assert f.kpdi_region_sums(h, ptr(r), 0, None) == 0
        assert not out.any()
        assert f.kpdi_region_sums(h, ptr(r), 1, ptr(out)) == 0 and np.array_equal(out[:, 0], data[:, :5, :5].sum(axis=(1, 2)))
