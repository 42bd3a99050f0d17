"""Axis reductions on the GPU (csrc/reduce.hip through kpdi_reduce_experimental, `pattern.reduce_stack`,
`EBSD.sum / mean / max / min / std / var`), held to the exact restatement and the per-value tolerances of
tests/_reduce_cases.py: every axis set, op and dtype; rows around the 16-byte vector; reduced and kept lengths around the
plan's slice and workgroup sizes; exact 64-bit integer sums; NaN and inf; residency; the reference's static-background
recipe."""

import ctypes as C
import os

import numpy as np
import pytest

import _reduce_cases as cases
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import reduce_stack
from kikuchipy_amd.signals import ReducedSignal

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reduced(s, op, axes):
    """`s.<op>` over the ARRAY axes `axes`, named in HyperSpy's order; the result's data in NumPy's shape."""
    nd = s.axes_manager.navigation_dimension
    out = getattr(s, op)(axis=cases.hyperspy_axes(axes, nd))
    if len(axes) == nd + 2:
        assert isinstance(out, ReducedSignal) and out.data.shape == (1,)
        return out.data.reshape(())
    assert isinstance(out, kpa.EBSD if max(axes) < nd else ReducedSignal)  # an EBSD while both detector axes survive
    return out.data


def check_all(data, axes_list=None, ops=cases.OPS, worst=None):
    """Every op over every axis set of `data` on a resident signal; prints the largest error / tolerance per op."""
    s = kpa.EBSD(data).to_device()
    try:
        for op in ops:
            ratio = 0.0
            for axes in axes_list or cases.subsets(data.ndim):
                ratio = max(ratio, cases.check(reduced(s, op, axes), data, op, axes))
            print(f"{data.dtype} {data.shape} {op}: largest error / tolerance {ratio:.3g}")
        assert s.is_resident
    finally:
        s._discard()


@pytest.mark.parametrize("ndim", [4, 3, 2])
@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_every_axis_set_op_and_dtype(dtype, ndim):
    check_all(cases.make_data(cases.SHAPES[ndim], dtype, seed=10 + ndim))


@pytest.mark.parametrize("dtype", cases.DTYPES)
def test_rows_around_the_vector(dtype):
    vec = 16 // np.dtype(dtype).itemsize
    for sx in (vec - 1, vec, vec + 1):  # an odd number of rows: they start at every alignment
        check_all(cases.make_data((2, 3, 3, sx), dtype, seed=sx), [(0, 1), (2,), (3,), (2, 3), (1, 3), (0, 2)], ("sum", "max", "var"))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_lengths_around_the_slice_and_the_workgroup(dtype):
    """Sizes read from the plan: the reduced length at slice - 1, slice, slice + 1 and 2 slice + 1 in both regimes, the
    kept inner length at one workgroup of vectors - 1, + 0, + 1 and two + 1."""
    cols = _lib.reduce_plan_describe(dtype, "sum", 1, 3, 1, 1, 40)  # axis 0 of (3, 1, 1, 40): the inner axis survives
    assert cols["regime"] == _lib.REDUCE_COLS
    for r in (cols["slice"] - 1, cols["slice"], cols["slice"] + 1, 2 * cols["slice"] + 1):
        check_all(cases.make_data((r, 2, 3, 5), dtype, seed=r), [(0,), (0, 2)], ("mean", "min", "std"))
    # the most slices that one lane combines, one more (16 lanes share them), and a count that leaves the 16 lanes uneven
    for slices in (_lib.REDUCE_COMBINE_SERIAL, _lib.REDUCE_COMBINE_SERIAL + 1, 3 * _lib.REDUCE_COMBINE_LANES + 5):
        r = (slices - 1) * cols["slice"] + 1
        plan = _lib.reduce_plan_describe(dtype, "sum", 1, r, 1, 2, 3)
        assert plan["n_slices"] == slices and plan["combine_lanes"] == (1 if slices <= _lib.REDUCE_COMBINE_SERIAL else 16)
        check_all(cases.make_data((r, 1, 2, 3), dtype, seed=slices), [(0,), (0, 3)])
    tile = _lib.REDUCE_THREADS * cols["vec"]
    for b in (tile - 1, tile, tile + 1, 2 * tile + 1):
        assert _lib.reduce_plan_describe(dtype, "sum", 1, 3, 1, 1, b)["grid_x"] == -(-b // tile)
        check_all(cases.make_data((3, 1, 1, b), dtype, seed=b), [(0,)], ("mean", "max", "var"))
    runs = _lib.reduce_plan_describe(dtype, "sum", 8, 2, 1, 1, 1 << 20)  # axis 3: runs, a whole wave per output
    assert runs["regime"] == _lib.REDUCE_RUNS and runs["group"] == 64
    for r in (runs["slice"] - 1, runs["slice"], runs["slice"] + 1, 2 * runs["slice"] + 1):
        assert _lib.reduce_plan_describe(dtype, "sum", 8, 2, 1, 1, r)["n_slices"] == -(-r // runs["slice"])
        check_all(cases.make_data((2, 1, 1, r), dtype, seed=r), [(3,), (0, 3)], ("mean", "min", "std"))


@pytest.mark.parametrize("shape", [(1, 1, 7, 9), (1, 6, 1, 9), (5, 1, 7, 1), (1, 1, 1, 1), (1, 9), (4, 1, 1)])
def test_single_element_axes(shape):
    for dtype in (np.int8, np.float64):
        check_all(cases.make_data(shape, dtype, seed=3), ops=("sum", "mean", "min", "var"))


@pytest.mark.parametrize("dtype, value", [(np.uint16, 65535), (np.int16, -32768)])
def test_sums_past_32_bits_are_exact(dtype, value):
    data = np.full((257, 257, 2, 3), value, dtype)  # 66 049 patterns: a 32-bit accumulator is wrong from 65 537 on
    s = kpa.EBSD(data).to_device()
    try:
        total, mean = s.sum(axis=(0, 1)), s.mean(axis=(0, 1))
        assert total.data.dtype == cases.result_dtype(dtype, "sum") and (total.data == 66049 * value).all()
        assert np.array_equal(total.data, data.sum(axis=(0, 1))) and np.array_equal(mean.data, data.mean(axis=(0, 1)))
        assert mean.data.dtype == np.float64 and (mean.data == value).all()
        assert (s.var(axis=(0, 1)).data == 0).all() and (s.std().data == 0).all()
        cases.check(s.sum(axis=(0, 1, 2, 3)).data.reshape(()), data, "sum", (0, 1, 2, 3))
    finally:
        s._discard()


def test_float32_of_alternating_sign():
    """sum|x| is 10^7 times |sum x|: the bound is relative to the former."""
    rng = np.random.default_rng(4)
    sign = np.where(np.indices((9, 11, 6, 7)).sum(axis=0) % 2, -1.0, 1.0)
    data = (sign * 3e7 + rng.standard_normal((9, 11, 6, 7))).astype(np.float32)
    check_all(data, [(0, 1), (2, 3), (3,), (0,), (0, 1, 2, 3), (1, 3)], ("sum", "mean", "std", "var"))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_and_inf_reach_exactly_their_windows(dtype):
    data = cases.make_data(cases.SHAPES[4], dtype, seed=8)
    data[1, 2, 3, 4] = np.nan
    data[3, 4, 5, 6] = np.inf
    with np.errstate(invalid="ignore"):
        want = data.sum(axis=(0, 1))
    assert np.isnan(want).sum() == 1 and np.isinf(want).sum() == 1  # (what `check` asks of every op and axis set)
    check_all(data)


def test_resident_and_host_backed_give_the_same_bits_twice():
    for dtype in (np.uint8, np.float32):
        data = cases.make_data((7, 5, 12, 10), dtype, seed=9)
        host = kpa.EBSD(data.copy())
        res = kpa.EBSD(data.copy()).to_device()
        try:
            for op in cases.OPS:
                for axes in [(0, 1), (2, 3), (1,), (3,), (0, 2), (0, 1, 2, 3)]:
                    a, b, c = reduced(host, op, axes), reduced(res, op, axes), reduced(res, op, axes)
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes() == c.tobytes(), (dtype, op, axes)
            assert res.is_resident and not host.is_resident
            assert np.array_equal(res.data, data) and np.array_equal(host.data, data)
        finally:
            res._discard()
            host.close()


def test_a_reduction_leaves_the_resident_patterns_alone():
    data = cases.make_data((4, 6, 20, 24), np.uint8, seed=11)
    s = kpa.EBSD(data.copy(), static_background=data[0, 0].copy()).to_device()
    try:
        s.remove_dynamic_background()  # (recorded; the host copy is stale from here on)
        assert s._host is None
        bg, image = s.mean(axis=(0, 1)), s.mean(axis=(2, 3))
        assert s.is_resident and s._host is None  # nothing was downloaded but the results
        assert isinstance(bg, kpa.EBSD) and not bg.is_resident and bg.data.shape == (20, 24)
        assert bg.static_background is s.static_background and bg.xmap is None
        assert isinstance(image, ReducedSignal) and image.data.shape == (4, 6)
        assert image.axes_manager.navigation_shape == (6, 4) and image.axes_manager.signal_shape == ()
        before = s.data.copy()
        for op in cases.OPS:
            getattr(s, op)(axis=(0, 3))
        assert np.array_equal(s._resident.host(), before) and s.is_resident
        # the host-backed chain
        h = kpa.EBSD(data.copy())
        h.remove_dynamic_background()
        assert np.array_equal(h.data, before)
        assert bg.data.tobytes() == h.mean(axis=(0, 1)).data.tobytes() == before.mean(axis=(0, 1)).tobytes()
        assert image.data.tobytes() == h.mean(axis=(2, 3)).data.tobytes() == before.mean(axis=(2, 3)).tobytes()
        h.close()
    finally:
        s._discard()


def test_detector_follows_the_navigation_shape():
    data = cases.make_data((2, 3, 8, 8), np.uint8, seed=12)
    pc = np.random.default_rng(0).random((2, 3, 3))
    s = kpa.EBSD(data, detector=kpa.EBSDDetector(shape=(8, 8), pc=pc))
    bg = s.mean(axis=(0, 1))
    assert bg.detector.navigation_shape == (1,) and np.allclose(bg.detector.pc[0], pc.reshape(-1, 3).mean(axis=0))
    assert bg.detector is not s.detector and s.detector.navigation_shape == (2, 3)
    row = s.max(axis="y")
    assert row.data.shape == (3, 8, 8) and row.detector.navigation_shape == (1,)
    with pytest.raises(ValueError, match="one GPU"):
        s.mean(axis=(0, 1), devices=[0, 0])
    s.close()


def test_the_references_static_background_recipe():
    """tests/test_signals/test_ebsd.py:489-494 of the reference, on a resident signal."""
    ni = np.load(os.path.join(GOLDEN, "h5ebsd_expected.npz"))["scan1"]
    whole = kpa.EBSD(ni.copy()).to_device()
    s = whole.isig[:, :-5]  # remove the bottom five rows
    whole._discard()
    try:
        assert s.is_resident and s.data.shape == (3, 3, 55, 60)
        static_bg = s.mean(axis=(0, 1))
        static_bg.change_dtype(np.uint8)
        s.remove_static_background(static_bg=static_bg.data)
        cropped = ni[:, :, :55]
        want_bg = cropped.mean(axis=(0, 1)).astype(np.uint8)
        assert static_bg.data.dtype == np.uint8 and np.array_equal(static_bg.data, want_bg)
        h = kpa.EBSD(cropped.copy())
        h.remove_static_background(static_bg=want_bg)
        assert s.is_resident and np.array_equal(s.data, h.data)
        h.close()
    finally:
        s._discard()


def test_block_wise_over_contexts():
    data = cases.make_data((3, 7, 12, 10), np.float32, seed=13)
    ctxs = [_lib.Context(0) for _ in range(2)]
    try:
        for op in ("mean", "std", "max"):
            for axes in [(2, 3), (3,), (2,)]:
                one, many = reduce_stack(data, op, axes), reduce_stack(data, op, axes, contexts=ctxs)
                assert one.shape == many.shape and one.tobytes() == many.tobytes()
                cases.check(many, data, op, axes)
        with pytest.raises(ValueError, match="one GPU"):
            reduce_stack(data, "mean", (0, 1), contexts=ctxs)
        cases.check(reduce_stack(data, "var", (0, -1), contexts=ctxs[:1]), data, "var", (0, 3))
    finally:
        for c in ctxs:
            c.close()


def test_refusals_of_the_entry_point_leave_the_context_usable():
    EINVAL = -1  # KPDI_EINVAL of include/kpdi.h
    data = cases.make_data((6, 8, 10), np.uint8, seed=14)
    with _lib.Context(0) as ctx:
        ctx.set_problem(8, 10, None, _lib.METRIC_NCC, 1)
        f, h = _lib.load(), ctx._h
        out = np.zeros((8, 10), dtype=np.float64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert f.kpdi_reduce_experimental(h, 1, 3, 2, 3, ptr(out), out.nbytes) == EINVAL  # no patterns yet
        ctx.set_experimental(data)
        for op, mask, ny, nx, nbytes, text in [(6, 3, 2, 3, 640, "unknown reduction op"), (-1, 3, 2, 3, 640, "unknown reduction op"),
                                               (1, 0, 2, 3, 640, "axis mask"), (1, 16, 2, 3, 640, "axis mask"),
                                               (1, 3, 2, 4, 640, "6 patterns are resident"), (1, 3, 0, 6, 640, "patterns are resident"),
                                               (1, 3, 2, 3, 639, "out_bytes"), (0, 3, 2, 3, 80, "out_bytes")]:
            assert f.kpdi_reduce_experimental(h, op, mask, ny, nx, ptr(out), nbytes) == EINVAL, (op, mask, ny, nx, nbytes)
            assert text in _lib.last_error(), _lib.last_error()
        assert f.kpdi_reduce_experimental(h, 1, 3, 2, 3, None, 640) == EINVAL
        assert not out.any()
        assert f.kpdi_reduce_experimental(h, 1, 3, 2, 3, ptr(out), out.nbytes) == 0
        assert np.array_equal(out, data.mean(axis=0))
        assert np.array_equal(ctx.reduce("sum", (0, 2), (6,)), data.sum(axis=(0, 2)))
        assert np.array_equal(ctx.get_experimental(), data)
