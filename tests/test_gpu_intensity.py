"""Intensity rescaling and normalization on the GPU (csrc/intensity.hip through kpdi_rescale_intensity /
kpdi_normalize_intensity / kpdi_intensity_range): against the reference's fixture (tests/golden/intensity.npz) and the
host restatement (tests/_intensity_restate.py), both kernel paths, the reference's known answers, dtype changes of the
resident patterns and what runs on them afterwards, block-wise runs over several contexts, and the EBSD methods."""

import json
import os

import numpy as np
import pytest

import _intensity_cases as cases
import _intensity_restate as R
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import (normalize_intensity, normalize_intensity_stack, rescale_intensity,
                                   rescale_intensity_stack)
from test_host_intensity import G, KNOWN_RESCALE, KNOWN_PERCENTILES, KNOWN_NORMALIZE, DUMMY, PRE, fixture_items

pytestmark = pytest.mark.gpu


def _norm_err(got, want):
    """(max |diff| over finite values, max relative diff, whether the NaN masks agree) of two float arrays."""
    g, w = got.astype(np.float64), want.astype(np.float64)
    fin = np.isfinite(w) & np.isfinite(g)
    d = np.abs(g - w)[fin]
    rel = d / np.maximum(np.abs(w[fin]), 1e-300)
    same = np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w))
    return (float(d.max()) if d.size else 0.0), (float(rel.max()) if rel.size else 0.0), same


def test_parity_with_the_reference():
    """Every fixture entry: rescale bit for bit (the int8 / int16 entries the reference's integer arithmetic wraps are
    exact against the restatement instead, and do differ from the fixture); normalize of integer patterns to float64
    within 1e-12 relative, of float patterns within 2e-5 absolute, integer outputs at most one level off."""
    worst = {}
    n_wrapped = 0
    for key, kind, name, flat, want in fixture_items():
        args = (cases.RESCALE if kind == "rescale" else cases.NORMALIZE)[name]
        if kind == "rescale":
            got = rescale_intensity_stack(flat, **args)[: len(want)]
            if not np.array_equal(got, want, equal_nan=want.dtype.kind == "f") or got.dtype != want.dtype:
                assert flat.dtype.kind == "i", key + " " + name
                exact = R.ebsd_rescale(flat, **args)[: len(want)]
                np.testing.assert_array_equal(got, exact, err_msg=f"{key} {name}")
                assert np.array_equal(R.ebsd_rescale(flat, wrap=True, **args)[: len(want)], want,
                                      equal_nan=want.dtype.kind == "f")
                n_wrapped += 1
            continue
        got = normalize_intensity_stack(flat, **args)[: len(want)]
        assert got.dtype == want.dtype, (key, name)
        src = "f32" if flat.dtype == np.float32 else ("f64" if flat.dtype == np.float64 else "int")
        tag = f"{src}->{want.dtype}"
        if want.dtype.kind == "f":
            ad, rd, same = _norm_err(got, want)
            assert same, (key, name)
            if src == "int" and want.dtype == np.float64:
                assert rd <= 1e-12, (key, name, rd)
            else:
                assert ad <= 2e-5 or rd <= 1e-6, (key, name, ad, rd)
            w = worst.setdefault(tag, {"max_abs": 0.0, "max_rel": 0.0})
            w["max_abs"], w["max_rel"] = max(w["max_abs"], ad), max(w["max_rel"], rd)
        else:
            d = np.abs(got.astype(np.int64) - want.astype(np.int64))
            # one level at a tie, or its wrapped image (0 <-> 255 for uint8 when the value is -0.x vs 0.x)
            span = 1 << (8 * want.dtype.itemsize)
            d = np.minimum(d, span - d)
            assert d.max() <= 1, (key, name, d.max())
            w = worst.setdefault(tag, {"max_levels": 0, "n_off": 0})
            w["max_levels"] = max(w["max_levels"], int(d.max()))
            w["n_off"] += int((d > 0).sum())
    assert n_wrapped > 0  # the documented int8 / int16 deviation is exercised
    out = os.environ.get("KPDI_INT_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"normalize": worst, "rescale": "bit-exact", "rescale_wrapped_entries": n_wrapped}, f, indent=1)


@pytest.mark.parametrize("shape, dtype", [((60, 60), "uint8"), ((61, 59), "int16"), ((240, 240), "float32"),
                                          ((90, 90), "float64"), ((1024, 1024), "uint8"), ((1024, 1024), "float64")])
def test_both_paths_agree(shape, dtype, monkeypatch):
    """The LDS path and the L2 path give the same bits for every mode (forced with KPDI_INTENSITY_PATH=1); both equal
    the restatement for rescale."""
    rng = np.random.default_rng(5)
    n = 2 if shape[0] > 500 else 5
    v = rng.random((n,) + shape) * 300 - 20
    p = cases.as_dtype(v if np.dtype(dtype).kind == "f" else np.clip(v, 0, 255), dtype)
    if np.dtype(dtype).kind == "f":
        p[0, 3, 4] = np.nan
    calls = [lambda: rescale_intensity_stack(p), lambda: rescale_intensity_stack(p, percentiles=(0.5, 99.5)),
             lambda: rescale_intensity_stack(p, relative=True, dtype_out=np.float32),
             lambda: rescale_intensity_stack(p, in_range=(10, 200), dtype_out=np.uint16),
             lambda: normalize_intensity_stack(p, dtype_out=np.float32)]
    first = [c() for c in calls]
    monkeypatch.setenv("KPDI_INTENSITY_PATH", "1")
    second = [c() for c in calls]
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    np.testing.assert_array_equal(first[0], R.ebsd_rescale(p))
    np.testing.assert_array_equal(first[1], R.ebsd_rescale(p, percentiles=(0.5, 99.5)))
    np.testing.assert_array_equal(first[2], R.ebsd_rescale(p, relative=True, dtype_out=np.float32))


def test_known_answers():
    """The reference's tests/test_signals/test_ebsd.py answers for its dummy signal, and its docstring's Ni answer."""
    for relative, dtype_out, answer in KNOWN_RESCALE:
        s = kpa.EBSD(DUMMY.copy())
        s.rescale_intensity(relative=relative, dtype_out=dtype_out, show_progressbar=True)
        assert s.data.dtype == answer.dtype
        assert np.allclose(s.data[0, 0], answer, atol=1e-4)
    for percentiles, answer in KNOWN_PERCENTILES:
        s = kpa.EBSD(DUMMY.astype(np.float32))
        s.rescale_intensity(percentiles=percentiles, dtype_out=np.uint8)
        assert s.data.dtype == np.uint8 and np.allclose(s.data[0, 0], answer, atol=2)
    for num_std, div, dtype_out, answer in KNOWN_NORMALIZE:
        s = kpa.EBSD(DUMMY.copy() if dtype_out is not None else DUMMY.astype(np.int16))
        s.normalize_intensity(num_std=num_std, divide_by_square_root=div, dtype_out=dtype_out, show_progressbar=True)
        assert s.data.dtype == (np.int16 if dtype_out is None else dtype_out)
        if dtype_out is not None:
            assert np.allclose(np.mean(s.data), 0, atol=1e-6)
        assert np.allclose(s.data[0, 0], answer, atol=1e-4)
    lo0, hi0, lo, hi = G["known__docstring_relative__ni_minmax"]
    s = kpa.EBSD(PRE["ni"].copy())
    s.rescale_intensity(relative=True)
    assert (s.data.min(), s.data.max(), s.data[0, 0].min(), s.data[0, 0].max()) == (lo0, hi0, lo, hi)


def test_single_pattern_functions():
    p = PRE["ni"][0, 0]
    np.testing.assert_array_equal(rescale_intensity(p), R.rescale(p))
    np.testing.assert_array_equal(rescale_intensity(p, out_range=(10, 245), dtype_out=np.float32),
                                  R.rescale(p, out_range=(10, 245), dtype_out=np.float32))
    # the whole input is one image: a 3-D stack shares one min / max
    st = PRE["ni"][0]
    one = rescale_intensity(st, percentiles=(1, 99))
    assert one.shape == st.shape
    np.testing.assert_array_equal(one, R.rescale(st.reshape(1, -1), percentiles=(1, 99)).reshape(st.shape))
    n = normalize_intensity(p)
    assert n.dtype == np.float64 and abs(n.mean()) < 1e-12 and abs(n.std() - 1) < 1e-12
    assert normalize_intensity(p.astype(np.float32)).dtype == np.float32
    assert normalize_intensity(p, dtype_out=np.uint8).dtype == np.uint8


@pytest.mark.parametrize("shape", [(60, 60), (240, 240)])
def test_resident_chain(shape):
    """uint8 -> static, dynamic background -> rescale_intensity(dtype_out=float32) on one context, then IQ, FFT filter
    and a dictionary sweep on the resident float32 patterns, equals the same steps after uploading the host-converted
    float32 patterns; and a float32 -> uint8 narrowing."""
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (20,) + shape).astype(np.uint8)
    bg = rng.integers(0, 40, shape).astype(np.uint8)
    dic = rng.random((300,) + shape).astype(np.float32)
    tf = kpa.filters.lowpass_fft_filter(shape, 22, 10)
    d, table = kpa.pattern._pattern.fft_filter_table(tf, "frequency", True, shape)

    def tail(ctx):
        iq = ctx.image_quality(True)
        ctx.fft_filter(d, table)
        ctx.reset_topk()
        ctx.push_dictionary_chunk(dic, 0)
        scores, idx = ctx.finalize(5)
        return iq, scores, idx, ctx.get_experimental()

    with _lib.Context(0) as ctx:
        ctx.set_problem(*shape, None, _lib.METRIC_NCC, 5)
        ctx.set_experimental(p)
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
        ctx.rescale_intensity(None, None, -1.0, 1.0, np.float32)
        converted = ctx.get_experimental()
        assert converted.dtype == np.float32
        a = tail(ctx)
        corrected = kpa.pattern.remove_dynamic_background(kpa.pattern.remove_static_background(p, bg))
        host = R.ebsd_rescale(corrected, dtype_out=np.float32)
        np.testing.assert_array_equal(converted, host)
        ctx.set_experimental(host)
        b = tail(ctx)
        # narrowing: float32 -> uint8 through the same resident buffer
        ctx.set_experimental(host)
        ctx.rescale_intensity(None, (1, 99), 0.0, 255.0, np.uint8)
        narrowed = ctx.get_experimental()
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    assert narrowed.dtype == np.uint8
    np.testing.assert_array_equal(narrowed, R.ebsd_rescale(host, percentiles=(1, 99), dtype_out=np.uint8))


@pytest.mark.parametrize("n_ctx", [2, 8])
def test_block_wise_over_contexts(n_ctx):
    rng = np.random.default_rng(3)
    p = rng.integers(0, 65535, (3, 7, 60, 60)).astype(np.uint16)
    p[1, 2] = 0
    f = p.astype(np.float32)
    f[2, 3, 5, 5] = np.nan
    calls = [(p, dict(relative=True)), (p, dict(percentiles=(1, 99), dtype_out=np.uint8)),
             (f, dict(relative=True, dtype_out=np.float64)), (f, dict(dtype_out=np.int16))]
    ctxs = [_lib.Context(0) for _ in range(n_ctx)]
    try:
        for data, kw in calls:
            one = rescale_intensity_stack(data, **kw)
            many = rescale_intensity_stack(data, contexts=ctxs, **kw)
            assert many.shape == data.shape and many.dtype == one.dtype
            assert np.array_equal(one, many, equal_nan=True)
        one = normalize_intensity_stack(p, dtype_out=np.float32)
        many = normalize_intensity_stack(p, dtype_out=np.float32, contexts=ctxs)
        assert np.isnan(one[1, 2]).all()  # the constant pattern: 0 / 0
        assert np.array_equal(one, many, equal_nan=True)
    finally:
        for c in ctxs:
            c.close()
    # relative with a NaN anywhere: every block is NaN (data.min() propagates NaN)
    assert np.isnan(rescale_intensity_stack(f, relative=True)).all()


@pytest.mark.parametrize("nav", [(), (5,), (2, 3)])
def test_ebsd_methods(nav):
    rng = np.random.default_rng(4)
    data = rng.integers(0, 256, nav + (60, 60)).astype(np.uint8)
    keep = data.copy()
    bg = rng.integers(0, 40, (60, 60)).astype(np.uint8)
    det = kpa.EBSDDetector(shape=(60, 60), pc=(0.4, 0.7, 0.5))
    s = kpa.EBSD(data, static_background=bg, detector=det)
    xmap = type("Map", (), {"shape": nav or (1,)})()
    s.xmap = xmap
    s2 = s.rescale_intensity(dtype_out=np.float32, inplace=False)
    assert np.array_equal(s.data, keep) and s.data is data  # not mutated
    assert isinstance(s2, kpa.EBSD) and s2.data.dtype == np.float32 and s2.data.shape == data.shape
    np.testing.assert_array_equal(s2.data, R.ebsd_rescale(keep.reshape((-1, 60, 60)), dtype_out=np.float32)
                                  .reshape(data.shape))
    assert np.array_equal(s2.static_background, bg) and s2.detector.shape == (60, 60)
    assert np.allclose(s2.detector.pc, det.pc) and s2.xmap is xmap
    s3 = s.normalize_intensity(dtype_out=np.float32, inplace=False, lazy_output=True)
    assert isinstance(s3, kpa.EBSD) and s3.data.dtype == np.float32 and s3.xmap is xmap
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        s.rescale_intensity(lazy_output=True)
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        s.normalize_intensity(lazy_output=True)
    # the tutorial's calls (pattern_processing.ipynb), in place, the dtype changing on the way
    assert s.rescale_intensity(relative=True) is None
    assert s.data.dtype == np.uint8
    s.rescale_intensity(out_range=(10, 245))
    s.rescale_intensity(percentiles=(0.5, 99.5))
    s.normalize_intensity(num_std=1, dtype_out=np.float32)
    assert s.data.dtype == np.float32 and s.data.shape == keep.shape
    assert s.xmap is xmap and s.detector is not None and np.array_equal(s.static_background, bg)
    s.rescale_intensity(dtype_out=np.uint8)
    assert s.data.dtype == np.uint8
