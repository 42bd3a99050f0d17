"""Downsampling and the dynamic background on the GPU (csrc/downsample.hip through kpdi_downsample, the
dynamic-background kernel of csrc/preproc.hip through kpdi_get_dynamic_background): against the reference's fixture
(tests/golden/downsample.npz) and the host restatement (tests/_downsample_restate.py), both kernel paths, the reference's
known answers and its TestDownsample / TestGetDynamicBackgroundEBSD behaviours through `kpa.EBSD`, block-wise runs over
several contexts, a resident chain at the C ABI and the refused calls.

Downsampling is bit-exact, with no tolerance and no excluded case.  The dynamic background follows the contract in
tests/test_host_downsample.py (`check_background`): integer results at most 1 level off on at most 1e-3 of the values,
float results within twice the restatement's measured distance to the reference plus 2^-24 max |value|."""

import json
import os

import numpy as np
import pytest

import _downsample_cases as cases
import _downsample_restate as R
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import downsample_stack, get_dynamic_background, get_dynamic_background_stack
from test_host_downsample import DUMMY, G, INPUTS, check_background, known

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_downsample_parity_with_the_reference():
    """Every fixture entry bit for bit: every input dtype, dtype_out, factor and shape, NaN positions included."""
    n = 0
    for name, factor, dtype_out in cases.downsample_cases():
        k = cases.key("ds", name, factor, dtype_out)
        got = downsample_stack(INPUTS[name], factor, dtype_out)
        want = G[k]
        assert same(got[: len(want)], want), k
        n += 1
    assert n == len(cases.downsample_cases()) > 100


def test_background_parity_with_the_reference():
    reached = {}
    for name, case, dtype_out in cases.background_cases():
        k = cases.key("bg", name, case, dtype_out)
        got = get_dynamic_background_stack(INPUTS[name], dtype_out=dtype_out, **cases.BACKGROUND[case])
        a, b = check_background(got, k)
        # the whole stack against the restatement: the same contract (the fixture stores the first pattern only)
        mine = R.get_dynamic_background(INPUTS[name], dtype_out=dtype_out, **cases.BACKGROUND[case])
        if got.dtype.kind == "f":
            d = float(np.max(np.abs(got.astype(np.float64) - mine.astype(np.float64))))
            assert d <= b, (k, d, b)
            reached[k] = {"max_abs_vs_reference": a, "bound": b, "max_abs_vs_restatement": d}
        else:
            diff = np.abs(got.astype(np.int64) - mine.astype(np.int64))
            assert diff.max() <= 1 and np.mean(diff != 0) <= 1e-3, k
            reached[k] = {"share_vs_reference": a, "max_levels": b, "share_vs_restatement": float(np.mean(diff != 0))}
            if cases.BACKGROUND[case]["filter_domain"] == "spatial":
                assert a == 0 and not diff.any(), k  # SciPy's order of operations and truncating stores, exactly
    out = os.environ.get("KPDI_DOWNSAMPLE_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"downsample": "bit-exact", "dynamic_background": reached}, f, indent=1)


@pytest.mark.parametrize("shape, dtype, factor", [((60, 60), "uint8", 2), ((60, 60), "float64", 3), ((120, 96), "int16", 4),
                                                  ((240, 240), "uint8", 4), ((480, 480), "uint16", 4),
                                                  ((480, 480), "uint8", 2), ((1024, 1024), "float64", 2)])
def test_both_paths_agree(shape, dtype, factor, monkeypatch):
    """The LDS path and the workspace path (forced with KPDI_DOWNSAMPLE_PATH=1, read at each call) give the same bits,
    those of the restatement; the last two shapes take the workspace path on their own."""
    rng = np.random.default_rng(6)
    n = 2 if shape[0] > 500 else 5
    v = rng.random((n,) + shape) * 300 - 20
    p = cases._intensity_cases.as_dtype(v if np.dtype(dtype).kind == "f" else np.clip(v, 0, 255), dtype)
    if np.dtype(dtype).kind == "f":
        p[1, 3, 4] = np.nan
    calls = [lambda: downsample_stack(p, factor), lambda: downsample_stack(p, factor, np.float32),
             lambda: downsample_stack(p, factor, np.uint16)]
    first = [c() for c in calls]
    monkeypatch.setenv("KPDI_DOWNSAMPLE_PATH", "1")
    second = [c() for c in calls]
    for a, b in zip(first, second):
        assert same(a, b)
    assert same(first[0], R.downsample_stack(p, factor))
    assert same(first[1], R.downsample_stack(p, factor, np.float32))
    assert same(first[2], R.downsample_stack(p, factor, np.uint16))


def test_known_answers():
    p = DUMMY[0, 0]
    for r in known("TestGetDynamicBackgroundPattern", "test_get_dynamic_background_pattern_spatial"):
        std = None if r["std"] is None else float(r["std"])
        bg = get_dynamic_background(p, filter_domain="spatial", std=std, truncate=float(r["truncate"]))
        assert bg.dtype == np.uint8 and np.allclose(bg, r["answer"])
    for r in known("TestGetDynamicBackgroundPattern", "test_get_dynamic_background_frequency"):
        a = r["answer"]
        bg = get_dynamic_background(p.astype(a.dtype), std=float(r["std"]))
        assert bg.dtype == a.dtype and np.allclose(bg, a, atol=1e-4)
    for r in known("TestGetDynamicBackgroundChunk", "test_get_dynamic_background_dtype_out"):
        a = r["answer"]
        s = kpa.EBSD(DUMMY.astype(a.dtype))
        bg = s.get_dynamic_background(std=2, dtype_out=a.dtype)
        assert bg.data.dtype == a.dtype and np.allclose(bg.data[0, 0], a, atol=1e-4)


@pytest.mark.parametrize("n_ctx", [2, 8])
def test_block_wise_over_contexts(n_ctx):
    rng = np.random.default_rng(3)
    p = rng.integers(0, 65535, (3, 7, 60, 60)).astype(np.uint16)
    p[1, 2] = 7
    f = p.astype(np.float32)
    f[2, 3, 5, 5] = np.nan
    ctxs = [_lib.Context(0) for _ in range(n_ctx)]
    try:
        for data, kw in [(p, dict(factor=2)), (p, dict(factor=3, dtype_out=np.uint8)), (f, dict(factor=4)),
                         (f, dict(factor=5, dtype_out=np.float64))]:
            one = downsample_stack(data, **kw)
            many = downsample_stack(data, contexts=ctxs, **kw)
            assert one.shape == data.shape[:2] + (60 // kw["factor"],) * 2 and same(one, many)
            assert same(one, R.downsample_stack(data, **kw))
        assert not one[1, 2].any() or np.isnan(one[1, 2]).all()
        for data, kw in [(p, dict(filter_domain="spatial")), (f, dict(std=3, truncate=3, dtype_out=np.int16))]:
            one = get_dynamic_background_stack(data, **kw)
            many = get_dynamic_background_stack(data, contexts=ctxs, **kw)
            assert one.shape == data.shape and same(one, many)
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("nav", [(), (5,), (2, 3)])
def test_ebsd_methods(nav):
    """The reference's TestDownsample (tests/test_signals/test_ebsd.py:2926-3000) and TestGetDynamicBackgroundEBSD."""
    rng = np.random.default_rng(4)
    data = rng.integers(0, 256, nav + (60, 48)).astype(np.uint8)
    keep = data.copy()
    bg = rng.integers(1, 40, (60, 48)).astype(np.uint8)
    det = kpa.EBSDDetector(shape=(60, 48), pc=(0.4, 0.7, 0.5), binning=2)
    s = kpa.EBSD(data, static_background=bg, detector=det)
    xmap = type("Map", (), {"shape": nav or (1,)})()
    s.xmap = xmap
    # not in place: a new signal, the original with its detector and background untouched
    s2 = s.downsample(2, inplace=False)
    assert s.data is data and np.array_equal(data, keep) and s.detector is det and det.shape == (60, 48)
    assert det.binning == 2 and s.static_background is bg
    assert isinstance(s2, kpa.EBSD) and s2.data.shape == nav + (30, 24) and s2.data.dtype == np.uint8
    assert same(s2.data, R.downsample_stack(keep, 2))
    assert s2.detector.shape == (30, 24) and s2.detector.binning == 4 and np.allclose(s2.detector.pc, det.pc)
    assert same(s2.static_background, R.downsample(bg, 2)) and s2.xmap is xmap
    assert s2.axes_manager.signal_shape == (24, 30)
    s3 = s.downsample(3, dtype_out="float32", inplace=False, lazy_output=True, show_progressbar=False)
    assert isinstance(s3, kpa.EBSD) and s3.data.dtype == np.float32 and s3.static_background.dtype == np.float32
    assert same(s3.data, R.downsample_stack(keep, 3, np.float32)) and same(s3.static_background, R.downsample(bg, 3, np.float32))
    assert np.allclose(s3.data.reshape(-1, 20 * 16).min(1), -1) and np.allclose(s3.data.reshape(-1, 20 * 16).max(1), 1)
    # the dynamic background: a new signal with the attributes carried over, the data untouched
    b = s.get_dynamic_background()
    assert isinstance(b, kpa.EBSD) and b.data.shape == data.shape and b.data.dtype == np.uint8 and s.data is data
    assert b.xmap is xmap and b.detector.shape == (60, 48) and np.array_equal(b.static_background, bg)
    want = R.get_dynamic_background(keep)
    diff = np.abs(b.data.astype(int) - want.astype(int))
    assert diff.max() <= 1 and np.mean(diff != 0) <= 1e-3
    b2 = s.get_dynamic_background("spatial", std=2, truncate=3, dtype_out=np.float32, lazy_output=True)
    assert b2.data.dtype == np.float32
    assert np.max(np.abs(b2.data - R.get_dynamic_background(keep, "spatial", 2, 3, np.float32))) <= 2.0 ** -24 * 255
    # in place (the default): data, detector and background follow; a second binning composes
    assert s.downsample(2) is None
    assert s.data.shape == nav + (30, 24) and same(s.data, s2.data) and s.detector.shape == (30, 24)
    assert s.detector.binning == 4 and same(s.static_background, s2.static_background) and s.xmap is xmap
    assert det.shape == (60, 48)  # the detector handed in is not mutated
    s.downsample(2, dtype_out=np.uint16)
    assert s.data.shape == nav + (15, 12) and s.data.dtype == np.uint16 and s.detector.binning == 8
    assert s.static_background.dtype == np.uint16 and s.static_background.shape == (15, 12)
    with pytest.raises(ValueError, match="Binning factor 2 must be a divisor of the initial pattern shape"):
        s.downsample(2)


@pytest.mark.parametrize("inplace", [True, False])
def test_detector_follows_without_one_set(inplace):
    """A signal built without a detector has the default one, as the reference's always has: it follows the binning too
    (shape, and binning 1 -> factor -> factor squared), whether or not `.detector` was read before."""
    rng = np.random.default_rng(8)
    s = kpa.EBSD(rng.integers(0, 256, (4, 60, 48)).astype(np.uint8))
    assert s._detector is None
    out = s.downsample(2, inplace=inplace)
    out = s if inplace else out
    assert out.detector.shape == (30, 24) and out.detector.binning == 2
    assert tuple(out.detector.unbinned_shape) == (60, 48)
    if not inplace:
        assert s.detector.shape == (60, 48) and s.detector.binning == 1
    out2 = out.downsample(2, inplace=inplace)
    out2 = out if inplace else out2
    assert out2.detector.shape == (15, 12) and out2.detector.binning == 4
    assert tuple(out2.detector.unbinned_shape) == (60, 48)
    out3 = out2.downsample(3, inplace=False)
    assert out3.detector.shape == (5, 4) and out3.detector.binning == 12 and out2.detector.binning == 4


def _sweep(ctx, dic):
    ctx.reset_topk()
    ctx.push_dictionary_chunk(dic, 0)
    return ctx.finalize(5)


def test_resident_chain_at_the_c_abi():
    """set_problem(120, 120) -> uint8 patterns -> a recorded static step -> kpdi_downsample(2, float32) -> a 60 x 60
    dictionary -> finalize equals, bit for bit, a fresh context given the downloaded binned patterns; a plain
    kpdi_set_problem with the new shape keeps the binned patterns, and so does one with a signal mask."""
    rng = np.random.default_rng(2)
    p = rng.integers(0, 256, (40, 120, 120)).astype(np.uint8)
    bg = rng.integers(0, 40, (120, 120)).astype(np.uint8)
    dic = rng.random((300, 60, 60)).astype(np.float32)
    mask = np.zeros((60, 60), dtype=bool)
    mask[:5] = True
    with _lib.Context(0) as ctx:
        ctx.set_problem(120, 120, None, _lib.METRIC_NCC, 5)
        ctx.set_experimental(p)
        ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
        ctx.downsample(2, np.float32)
        a = _sweep(ctx, dic)
        binned = ctx.get_experimental()
        assert binned.shape == (40, 60, 60) and binned.dtype == np.float32
        assert same(binned, R.downsample_stack(kpa.pattern.remove_static_background(p, bg), 2, np.float32))
        ctx.set_problem(60, 60, None, _lib.METRIC_NCC, 5)  # the new shape: the binned patterns stay resident
        assert ctx.n_experimental == 40
        a2 = _sweep(ctx, dic)
        ctx.set_problem(60, 60, mask, _lib.METRIC_NCC, 5)
        assert ctx.n_experimental == 40
        am = _sweep(ctx, dic)
        assert same(ctx.get_experimental(), binned)
    with _lib.Context(0) as ctx:
        ctx.set_problem(60, 60, None, _lib.METRIC_NCC, 5)
        ctx.set_experimental(binned)
        b = _sweep(ctx, dic)
        ctx.set_problem(60, 60, mask, _lib.METRIC_NCC, 5)
        bm = _sweep(ctx, dic)
    for x, y in zip(a + a2 + am, b + b + bm):
        assert np.array_equal(x, y)


def test_refused_calls_leave_the_resident_set():
    rng = np.random.default_rng(7)
    p = rng.integers(0, 256, (6, 60, 48)).astype(np.uint8)
    mask = np.zeros((60, 48), dtype=bool)
    mask[0] = True
    with _lib.Context(0) as ctx:
        ctx.set_problem(60, 48, None, _lib.METRIC_NCC, 5)
        with pytest.raises(_lib.KpdiError):  # no resident patterns
            ctx.downsample(2, np.uint8)
        assert ctx._detector == (60, 48)
        ctx.set_experimental(p)

        def untouched():
            """The wrapper's own view of the resident set, and the set itself."""
            assert (ctx._detector, ctx._exp_shape, ctx._exp_dtype) == ((60, 48), (6, 60, 48), np.dtype(np.uint8))
            assert ctx.n_experimental == 6 and same(ctx.get_experimental(), p)

        for factor, dt in [(1, None), (0, None), (-2, None), (5, None), (7, None), (2, np.float16), (2, np.int32)]:
            with pytest.raises(_lib.KpdiError):
                ctx.downsample(factor, dt)
            untouched()
        with pytest.raises(_lib.KpdiError):
            ctx.get_dynamic_background(7, None, 4.0)  # unknown domain
        with pytest.raises(_lib.KpdiError):
            ctx.get_dynamic_background(_lib.DOMAIN_FREQUENCY, 0.1, 4.0)  # an empty window
        ctx.hold_dictionary_chunk(rng.random((50, 60, 48)).astype(np.float32), 0)  # held chunks of the old shape
        ctx.synchronize()
        with pytest.raises(_lib.KpdiError, match="held"):
            ctx.downsample(2)
        untouched()
        ctx.release_held()
        ctx.set_problem(60, 48, mask, _lib.METRIC_NCC, 5)  # a signal mask of the old shape
        with pytest.raises(_lib.KpdiError, match="signal mask"):
            ctx.downsample(2)
        untouched()
        ctx.set_problem(60, 48, None, _lib.METRIC_NCC, 5)
        ctx.downsample(2)
        assert same(ctx.get_experimental(), R.downsample_stack(p, 2))
        # the background only reads the resident patterns
        before = ctx.get_experimental()
        bgd = ctx.get_dynamic_background(_lib.DOMAIN_SPATIAL, None, 4.0, np.float32)
        assert bgd.shape == (6, 30, 24) and bgd.dtype == np.float32 and same(ctx.get_experimental(), before)
