"""Image quality on the GPU (csrc/iq.hip through kpdi_image_quality): against the reference's fixture
(tests/golden/image_quality.npz) and the float64 restatement of test_host_image_quality.py for every shape and dtype,
the reference's known answers, degenerate patterns, resident (background-corrected) patterns, block-wise runs over
several contexts, and the EBSD method."""

import json
import os

import numpy as np
import pytest

import _iq_inputs
import kikuchipy_amd as kpa
from conftest import GOLDEN
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import get_image_quality
from test_host_image_quality import DUMMY_NORM, DUMMY_RAW, IQ, fixture_cases, iq_f64

pytestmark = pytest.mark.gpu

# |Q_gpu - Q_reference| bound: f32 DFT sums of up to 240 terms per pass
TOL = 1e-5
# 1001 x 1001: each pass sums 1001 f32 terms (a direct DFT, no FFT's log-depth tree): the rounding of a coefficient grows
# with the length of its sums, about 4x that of 240, and Q averages half a million of them
TOL_LARGE = 1e-4


def test_parity_with_the_reference_and_the_restatement():
    worst = {}
    with _lib.Context(0) as ctx:
        for key, stack, norm, kw in fixture_cases():
            got = get_image_quality(stack, bool(norm), context=ctx, **kw)
            got = np.asarray(got)
            assert got.dtype == np.float32 and got.shape == IQ[key].shape, key
            tol = TOL_LARGE if stack.shape[-1] > 240 else TOL
            d_ref = float(np.max(np.abs(got - IQ[key])))
            d_f64 = float(np.max(np.abs(got - iq_f64(stack, bool(norm), **kw))))
            worst[key] = (d_ref, d_f64)
            assert d_ref <= tol and d_f64 <= tol, (key, d_ref, d_f64)
    out = os.environ.get("KPDI_IQ_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump(worst, f, indent=1)
    small = max(max(v) for k, v in worst.items() if "1001" not in k)
    large = max(max(v) for k, v in worst.items() if "1001" in k)
    print(f"largest |dQ| up to 240x240: {small:.3g}; 1001x1001: {large:.3g}")


def test_one_pattern_is_a_float():
    d = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    q = get_image_quality(d[0, 0])
    assert isinstance(q, float) and abs(q - -0.0241) < 1e-4
    assert abs(get_image_quality(d[0, 0], normalize=False) - 0.2694) < 1e-4
    assert abs(get_image_quality(d[2, 2]) - -0.2385) < 1e-4


def test_known_answers_dummy_maps():
    d = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
    s = kpa.EBSD(d.copy())
    assert np.allclose(s.get_image_quality(), DUMMY_NORM, atol=1e-4)
    assert np.allclose(s.get_image_quality(normalize=False), DUMMY_RAW, atol=1e-4)


def test_white_noise_and_flat_1001():
    rng = np.random.default_rng(0)
    assert abs(get_image_quality(rng.random((1001, 1001)))) < 1e-2
    assert abs(get_image_quality(np.full((1001, 1001), 5.0), normalize=False) - 1) < 1e-2


@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])  # both kernel paths
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.float64])
def test_degenerate_patterns(shape, dtype):
    rng = np.random.default_rng(5)
    p = (rng.random((8,) + shape) * 100).astype(dtype)
    p[1] = 0           # black frame
    p[2] = 37          # constant, not zero
    if np.issubdtype(dtype, np.floating):
        p[3, 4, 5] = np.nan
        p[4, 0, 0] = np.inf
        p[5, -1, -1] = -np.inf
    for norm in (True, False):
        q = get_image_quality(p, norm)
        nan = np.isnan(q)
        want = {1, 3, 4, 5} if np.issubdtype(dtype, np.floating) else {1}
        if norm:
            want = want | {2}
        assert set(np.flatnonzero(nan)) == want, (norm, np.flatnonzero(nan))
        ok = [i for i in range(8) if i not in want]
        assert np.all(np.isfinite(q[ok]))
        assert np.max(np.abs(q[ok] - iq_f64(p[ok], norm))) <= TOL
        if not norm:  # a constant pattern: only F(0, 0) is non-zero
            assert abs(q[2] - (1 - 1 / (np.sum(kpa.pattern.fft_frequency_vectors(shape)) / p[0].size))) < 1e-6


@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
def test_resident_patterns_after_background_removal(shape):
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (20,) + shape).astype(np.uint8)
    bg = rng.integers(0, 40, shape).astype(np.uint8)
    with _lib.Context(0) as ctx:
        ctx.set_problem(*shape, None, _lib.METRIC_NCC, 1)
        ctx.set_experimental(p.reshape(-1, *shape))
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
        for norm in (True, False):
            resident = ctx.image_quality(norm)
            corrected = ctx.get_experimental()
            again = get_image_quality(corrected, norm, context=ctx)
            assert np.array_equal(resident, again, equal_nan=True)
    s = kpa.EBSD(p.copy(), static_background=bg)
    s.remove_static_background()
    s.remove_dynamic_background()
    assert np.array_equal(s.get_image_quality(), get_image_quality(s.data))


@pytest.mark.parametrize("n_ctx", [2, 8])
@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
def test_block_wise_over_contexts(n_ctx, shape):
    rng = np.random.default_rng(3)
    p = rng.integers(0, 65535, (3, 7) + shape).astype(np.uint16)
    p[1, 2] = 0
    one = get_image_quality(p)
    ctxs = [_lib.Context(0) for _ in range(n_ctx)]
    try:
        many = get_image_quality(p, contexts=ctxs)
    finally:
        for c in ctxs:
            c.close()
    assert many.shape == (3, 7) and many.dtype == np.float32
    assert np.array_equal(one, many, equal_nan=True)


@pytest.mark.parametrize("nav", [(), (5,), (2, 3)])
def test_ebsd_method_shapes_and_no_mutation(nav):
    rng = np.random.default_rng(4)
    data = rng.integers(0, 256, nav + (60, 60)).astype(np.uint8)
    keep = data.copy()
    s = kpa.EBSD(data)
    q = s.get_image_quality()
    assert isinstance(q, np.ndarray) and q.shape == nav and q.dtype == np.float32
    assert np.array_equal(s.data, keep) and s.data is data
    assert np.allclose(q, iq_f64(keep), atol=TOL, rtol=0)
    q2 = s.get_image_quality(normalize=False, show_progressbar=False)
    assert q2.shape == nav and np.allclose(q2, iq_f64(keep, False), atol=TOL, rtol=0)
