"""The FFT filter on the GPU (csrc/fftfilter.hip through kpdi_fft_filter): against the reference's fixture
(tests/golden/fft_filter.npz) and the float64 restatement of test_host_fft_filter.py for every shape and dtype in both
domains, the reference's known answers on its dummy signal, degenerate patterns, resident (background-corrected)
patterns and what runs on them afterwards, block-wise runs over several contexts, and the EBSD method."""

import json
import os

import numpy as np
import pytest

import _fft_filter_cases as cases
import _iq_inputs
import kikuchipy_amd as kpa
from conftest import GOLDEN
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import fft_filter_stack
from test_host_fft_filter import FF, OURS, assert_close, case_f64, filter_f64, synthetic_keys, tie_fraction

pytestmark = pytest.mark.gpu

FLOAT_TOL = 1e-5   # float outputs (range [-1, 1]) against the reference and the restatement
INT_FRAC = 1e-3    # integer outputs against the restatement: one grey level apart on at most this fraction of pixels
DUMMY = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]
PRE = np.load(os.path.join(GOLDEN, "preproc.npz"))


def gpu_case(stack, name, ctx):
    domain, shift, build = cases.CASES[name]
    return fft_filter_stack(stack, build(stack.shape[-2:], OURS), domain, shift, context=ctx)


def diff(got, want):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    return float(np.nanmax(d)), float(np.count_nonzero(d) / d.size)


def frac_for(dtype, base):
    """uint16: one grey level is 1.5e-5 of the range, below what f32 DFT sums resolve on every pixel (measured up to
    0.5 % of the pixels one level off at 128 x 96); uint8 and float32: `base`."""
    return max(base, 2e-2) if np.dtype(dtype) == np.uint16 else base


def record(name, data):
    out = os.environ.get("KPDI_FF_PARITY_OUT")
    if out:
        with open(out.replace(".json", f"_{name}.json"), "w") as f:
            json.dump(data, f, indent=1)


def check_all(checks):
    """Run every (label, got, want, int_frac, atol) comparison, record the measured maxima, then fail on the first."""
    worst, failed = {}, []
    for label, got, want, frac, atol in checks:
        worst[label] = diff(got, want)
        try:
            assert_close(got, want, label, frac_for(got.dtype, frac), atol=atol)
        except AssertionError as e:
            failed.append(str(e)[:300])
    return worst, failed


def test_parity_with_the_reference():
    checks = []
    with _lib.Context(0) as ctx:
        for name in cases.NAMES:
            frac = tie_fraction(name)
            checks.append((f"ni__{name}", gpu_case(PRE["ni"], name, ctx), FF[f"ni__{name}"], frac, FLOAT_TOL))
            if name in cases.NI_CORRECTED_CASES:
                key = f"ni_corrected__{name}"
                checks.append((key, gpu_case(PRE["ni__static_then_dynamic"], name, ctx), FF[key], frac, FLOAT_TOL))
            for dtype in _iq_inputs.DTYPES:
                key = f"dummy__{dtype}__{name}"
                checks.append((key, gpu_case(DUMMY.astype(dtype), name, ctx), FF[key], 8 / 81, FLOAT_TOL))
        for key in synthetic_keys():
            _, shape, dtype = key.split("__")
            shape = tuple(int(v) for v in shape.split("x"))
            stack = _iq_inputs.stack(shape, dtype, int(FF[key + "__seed"]))[: cases.N_STORED]
            name = str(FF[key + "__case"])
            frac = 5e-2 if shape == (1, 64) else tie_fraction(name)
            checks.append((key, gpu_case(stack, name, ctx), FF[key], frac, FLOAT_TOL))
    worst, failed = check_all(checks)
    record("reference", worst)
    assert not failed, failed


@pytest.mark.parametrize("shape", _iq_inputs.SHAPES)
def test_parity_with_the_restatement_for_every_shape(shape):
    """Every shape of _iq_inputs up to 1001 x 1001 (the LDS path and the workspace path), both domains, three dtypes."""
    checks = []
    with _lib.Context(0) as ctx:
        for di, dtype in enumerate(_iq_inputs.DTYPES):
            stack = _iq_inputs.stack(shape, dtype, 7000 + di)
            for name in ("lowhigh", "complex", "gauss5", "even4"):
                checks.append((f"{dtype}__{name}", gpu_case(stack, name, ctx), case_f64(stack, name), INT_FRAC,
                               FLOAT_TOL))
    worst, failed = check_all(checks)
    record(f"restatement_{shape[0]}x{shape[1]}", worst)
    assert not failed, failed


# the reference's tests/test_signals/test_ebsd.py:1934-2009 on its dummy signal
@pytest.mark.parametrize("shift, tf, dtype, spectrum_sum", [
    (True, lambda: np.outer(kpa.filters.modified_hann(3), kpa.filters.modified_hann(3)), np.float32, 5.2000),
    (True, lambda: kpa.filters.lowpass_fft_filter((3, 3), 30, 15), np.float64, 6.1428),
    (False, lambda: kpa.filters.highpass_fft_filter((3, 3), 2, 1), np.float32, 5.4155),
    (False, lambda: kpa.filters.Window("gaussian", (3, 3), std=2), np.float32, 6.2621),
])
def test_known_answers_frequency(shift, tf, dtype, spectrum_sum):
    s = kpa.EBSD(DUMMY.astype(dtype))
    s.fft_filter(transfer_function=tf(), function_domain="frequency", shift=shift, show_progressbar=True)
    assert isinstance(s, kpa.EBSD) and s.data.dtype == dtype
    # the reference's fft_spectrum of the (real) filtered pattern is its magnitude, element-wise
    assert np.isclose(np.sum(np.abs(s.data[0, 0])), spectrum_sum, atol=1e-4)


def test_known_answer_spatial_sobel():
    from scipy.ndimage import correlate

    s = kpa.EBSD(DUMMY.astype(np.float32))
    p = s.data[0, 0].copy()
    w = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]])
    s.fft_filter(transfer_function=w, function_domain="spatial", shift=False)
    p2 = s.data[0, 0]
    assert not np.allclose(p, p2, atol=1e-1)
    p3 = correlate(p, w.astype(np.float32), mode="nearest")
    p3 = (p3 - p3.min()) / (p3.max() - p3.min()) * 2 - 1
    assert np.allclose(p2, p3)


@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
@pytest.mark.parametrize("name", ["lowhigh", "gauss5"])
def test_degenerate_patterns(shape, name):
    """Constant, all-zero and non-finite patterns: 0 for integer dtypes, NaN for float dtypes; the others untouched."""
    rng = np.random.default_rng(1)
    u = rng.integers(0, 256, (4,) + shape).astype(np.uint8)
    u[0] = 0
    u[1] = 77
    f = rng.random((5,) + shape).astype(np.float32)
    f[0] = 0
    f[1] = 0.25
    f[2, 3, 4] = np.nan
    f[3, 0, 0] = np.inf
    with _lib.Context(0) as ctx:
        gu = gpu_case(u, name, ctx)
        gf = gpu_case(f, name, ctx)
    assert (gu[:2] == 0).all()
    assert np.isnan(gf[:4]).all() and np.isfinite(gf[4]).all()
    assert gu.shape == u.shape and gu.dtype == u.dtype and gf.dtype == f.dtype
    # all zero: the reference's 0 / 0 as well; a constant non-zero pattern is defined as degenerate here, where the
    # reference rescales its FFT's round-off
    np.testing.assert_array_equal(gu[:1], case_f64(u[:1], name))
    assert np.isnan(case_f64(f[2:4], name)).all()
    assert diff(gu[2:], case_f64(u[2:], name))[0] <= 1


@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
@pytest.mark.parametrize("name", ["lowhigh", "gauss5"])
def test_resident_chain(shape, name):
    """static -> dynamic -> fft_filter -> get_experimental on one context equals the same steps with a download and an
    upload between them; image quality and a dictionary sweep on the filtered resident patterns equal the same calls on
    the downloaded array."""
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (20,) + shape).astype(np.uint8)
    bg = rng.integers(0, 40, shape).astype(np.uint8)
    dic = rng.random((300,) + shape).astype(np.float32)
    domain, shift, build = cases.CASES[name]
    tf = build(shape, OURS)
    d, table = kpa.pattern._pattern.fft_filter_table(tf, domain, shift, shape)
    with _lib.Context(0) as ctx:
        ctx.set_problem(*shape, None, _lib.METRIC_NCC, 5)
        ctx.set_experimental(p)
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
        ctx.fft_filter(d, table)
        iq_resident = ctx.image_quality(True)
        ctx.reset_topk()
        ctx.push_dictionary_chunk(dic, 0)
        scores, idx = ctx.finalize(5)
        resident = ctx.get_experimental()
    with _lib.Context(0) as ctx:
        ctx.set_problem(*shape, None, _lib.METRIC_NCC, 5)
        ctx.set_experimental(p)
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
        corrected = ctx.get_experimental()
        ctx.set_experimental(corrected)
        ctx.fft_filter(d, table)
        stepwise = ctx.get_experimental()
        ctx.set_experimental(stepwise)
        iq_again = ctx.image_quality(True)
        ctx.reset_topk()
        ctx.push_dictionary_chunk(dic, 0)
        scores2, idx2 = ctx.finalize(5)
    assert np.array_equal(resident, stepwise)
    assert np.array_equal(iq_resident, iq_again, equal_nan=True)
    assert np.array_equal(scores, scores2) and np.array_equal(idx, idx2)
    assert np.array_equal(resident, fft_filter_stack(corrected, tf, domain, shift))


@pytest.mark.parametrize("n_ctx", [2, 8])
@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
def test_block_wise_over_contexts(n_ctx, shape):
    rng = np.random.default_rng(3)
    p = rng.integers(0, 65535, (3, 7) + shape).astype(np.uint16)
    p[1, 2] = 0
    for name in ("lowhigh", "sobel"):
        domain, shift, build = cases.CASES[name]
        tf = build(shape, OURS)
        one = fft_filter_stack(p, tf, domain, shift)
        ctxs = [_lib.Context(0) for _ in range(n_ctx)]
        try:
            many = fft_filter_stack(p, tf, domain, shift, contexts=ctxs)
        finally:
            for c in ctxs:
                c.close()
        assert many.shape == p.shape and many.dtype == np.uint16
        assert np.array_equal(one, many)


@pytest.mark.parametrize("nav", [(), (5,), (2, 3)])
def test_ebsd_method(nav):
    rng = np.random.default_rng(4)
    data = rng.integers(0, 256, nav + (60, 60)).astype(np.uint8)
    keep = data.copy()
    w = kpa.filters.lowpass_fft_filter((60, 60), 22, 10) * kpa.filters.highpass_fft_filter((60, 60), 1, 0.5)
    bg = rng.integers(0, 40, (60, 60)).astype(np.uint8)
    det = kpa.EBSDDetector(shape=(60, 60), pc=(0.4, 0.7, 0.5))
    s = kpa.EBSD(data, static_background=bg, detector=det)
    xmap = type("Map", (), {"shape": nav or (1,)})()
    s.xmap = xmap
    s2 = s.fft_filter(w, "frequency", shift=True, inplace=False)
    assert np.array_equal(s.data, keep) and s.data is data  # not mutated
    assert isinstance(s2, kpa.EBSD) and s2.data.dtype == np.uint8 and s2.data.shape == data.shape
    want = filter_f64(keep, "frequency", True, w)
    assert diff(s2.data, want)[0] <= 1
    assert np.array_equal(s2.static_background, bg) and s2.detector.shape == (60, 60)
    assert np.allclose(s2.detector.pc, det.pc) and s2.xmap is xmap
    s3 = s.fft_filter(w, "frequency", True, None, False, True)  # lazy_output=True with inplace=False: a new signal
    assert isinstance(s3, kpa.EBSD) and np.array_equal(s3.data, s2.data)
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        s.fft_filter(w, "frequency", lazy_output=True)
    with pytest.raises(ValueError, match=r"must be either of \['frequency', 'spatial'\]"):
        s.fft_filter(w, "fourier")
    assert s.fft_filter(np.ones((3, 3)), "spatial") is None  # in place
    assert s.data.dtype == np.uint8 and s.data.shape == keep.shape
    assert np.array_equal(s.data, fft_filter_stack(keep, np.ones((3, 3)), "spatial"))
