"""Adaptive histogram equalization on the GPU (csrc/clahe.hip through kpdi_adaptive_histogram_equalization): bit for bit
against the reference's fixture (tests/golden/clahe.npz) and the host restatement (tests/_clahe_restate.py), both
kernel paths, large patterns and kernels of one pixel, a resident chain into dictionary indexing, block-wise runs over
several contexts, and the EBSD method."""

import numpy as np
import pytest

import _clahe_cases as cases
import _clahe_restate as R
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import adaptive_histogram_equalization, adaptive_histogram_equalization_stack
from test_host_clahe import PRE, fixture_items

pytestmark = pytest.mark.gpu


def test_parity_with_the_reference():
    n = 0
    for key, name, flat, want in fixture_items():
        kernel, clip, nbins = cases.args(name)
        got = adaptive_histogram_equalization_stack(flat[: len(want)], kernel, clip, nbins)
        assert got.dtype == want.dtype, (key, name)
        np.testing.assert_array_equal(got, want, err_msg=f"{key} {name}")
        n += 1
    assert n > 90


def _stack(shape, dtype, n, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[: shape[0], : shape[1]]
    ramp = ((3 * y + 5 * x) % 97) / 96.0
    v = 0.6 * rng.random((n,) + shape) + 0.4 * ramp
    return cases.as_dtype(np.floor(v * 65535).astype(np.uint16), dtype)


@pytest.mark.parametrize("shape, dtype, kernel, clip, nbins", [
    ((60, 60), "uint8", None, 0, 128), ((60, 60), "uint8", None, 0.01, 128), ((61, 59), "int16", (7, 13), 0.01, 64),
    ((240, 240), "float32", (1, 1), 0, 128), ((90, 90), "float64", 10, 0.05, 256), ((64, 96), "uint16", (80, 80), 1.0, 16384),
    ((128, 128), "int8", (3, 5), 0.02, 1)])
def test_both_paths_agree(shape, dtype, kernel, clip, nbins, monkeypatch):
    """The LDS path and the workspace path (KPDI_CLAHE_PATH=1, several bands) give the same bits, equal to the
    restatement."""
    p = _stack(shape, dtype, 3, 5)
    if np.dtype(dtype).kind == "f":
        p[0, 3, 4] = np.nan
    first = adaptive_histogram_equalization_stack(p, kernel, clip, nbins)
    monkeypatch.setenv("KPDI_CLAHE_PATH", "1")
    second = adaptive_histogram_equalization_stack(p, kernel, clip, nbins)
    assert first.dtype == second.dtype == p.dtype
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first, R.ebsd_equalize(p, kernel, clip, nbins))


@pytest.mark.parametrize("shape, kernel, clip, nbins", [
    ((1024, 1024), None, 0.01, 128), ((1024, 1024), (2, 2), 0, 64), ((240, 240), (1, 1), 0, 128),
    ((240, 240), (1, 1), 0.5, 16384)])
def test_large_patterns_and_one_pixel_kernels(shape, kernel, clip, nbins):
    p = _stack(shape, "uint8", 1 if shape[0] > 500 else 2, 6)
    got = adaptive_histogram_equalization_stack(p, kernel, clip, nbins)
    np.testing.assert_array_equal(got, R.ebsd_equalize(p, kernel, clip, nbins))


def test_single_pattern_function():
    p = PRE["ni"][0, 0]
    got = adaptive_histogram_equalization(p, None)  # scikit-image's default: (sy // 8, sx // 8)
    np.testing.assert_array_equal(got, R.equalize(p, 7, 7))
    got = adaptive_histogram_equalization(p, (7, 13), clip_limit=0.01, nbins=64)
    np.testing.assert_array_equal(got, R.equalize(p, 7, 13, 0.01, 64))
    f = (p / 255.0).astype(np.float32)
    np.testing.assert_array_equal(adaptive_histogram_equalization(f, 10), R.equalize(f, 10, 10))


def test_resident_chain():
    """static, then dynamic background, then CLAHE on one context, then a dictionary sweep on the resident patterns,
    equals the same steps with downloads in between."""
    shape = (60, 60)
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (20,) + shape).astype(np.uint8)
    bg = rng.integers(0, 40, shape).astype(np.uint8)
    dic = rng.random((300,) + shape).astype(np.float32)

    def tail(ctx):
        ctx.reset_topk()
        ctx.push_dictionary_chunk(dic, 0)
        scores, idx = ctx.finalize(5)
        return scores, idx

    with _lib.Context(0) as ctx:
        ctx.set_problem(*shape, None, _lib.METRIC_NCC, 5)
        ctx.set_experimental(p)
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
        ctx.adaptive_histogram_equalization(15, 15, 2, 128)  # clip_limit=0.01
        resident = ctx.get_experimental()
        a = tail(ctx)
        corrected = kpa.pattern.remove_dynamic_background(kpa.pattern.remove_static_background(p, bg))
        host = adaptive_histogram_equalization_stack(corrected, None, 0.01)
        np.testing.assert_array_equal(resident, host)
        np.testing.assert_array_equal(host, R.ebsd_equalize(corrected, None, 0.01))
        ctx.set_experimental(host)
        b = tail(ctx)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("n_ctx", [1, 2, 8])
def test_block_wise_over_contexts(n_ctx):
    p = _stack((60, 60), "uint16", 21, 3).reshape(3, 7, 60, 60)
    p[1, 2] = 0
    one = adaptive_histogram_equalization_stack(p, None, 0.01)
    ctxs = [_lib.Context(0) for _ in range(n_ctx)]
    try:
        many = adaptive_histogram_equalization_stack(p, None, 0.01, contexts=ctxs)
    finally:
        for c in ctxs:
            c.close()
    assert many.shape == p.shape and many.dtype == p.dtype
    np.testing.assert_array_equal(one, many)


@pytest.mark.parametrize("nav", [(), (5,), (2, 3)])
def test_ebsd_method(nav):
    rng = np.random.default_rng(4)
    data = rng.integers(0, 256, nav + (60, 60)).astype(np.uint8)
    keep = data.copy()
    bg = rng.integers(0, 40, (60, 60)).astype(np.uint8)
    det = kpa.EBSDDetector(shape=(60, 60), pc=(0.4, 0.7, 0.5))
    s = kpa.EBSD(data, static_background=bg, detector=det)
    want = R.ebsd_equalize(keep)
    s2 = s.adaptive_histogram_equalization(inplace=False)
    assert np.array_equal(s.data, keep) and s.data is data  # not mutated
    assert isinstance(s2, kpa.EBSD) and s2.data.dtype == np.uint8 and s2.data.shape == data.shape
    np.testing.assert_array_equal(s2.data, want)
    assert np.array_equal(s2.static_background, bg) and s2.detector.shape == (60, 60)
    s3 = s.adaptive_histogram_equalization(kernel_size=10, clip_limit=0.01, nbins=64, inplace=False, lazy_output=True)
    np.testing.assert_array_equal(s3.data, R.ebsd_equalize(keep, 10, 0.01, 64))
    # the tutorial's calls (pattern_processing.ipynb): background removal, then equalization in place
    assert s.adaptive_histogram_equalization() is None
    np.testing.assert_array_equal(s.data, want)
    assert s.detector is not None and np.array_equal(s.static_background, bg)
