"""BASELINE.json configs[2]: signal mask + static/dynamic background removal FUSED with the
preparation of the patterns (csrc/preproc.hip: preproc_fused_kernel), then the match.

* fused == step by step, bit for bit on the pre-processed patterns (both quantisations kept);
* detectors beyond the LDS limit of the fused kernel (raw 480 x 480 patterns) take the streaming
  kernels and meet the same contract;
* the whole workload at full size (4096 x 100 000, K = 2819): >= 256 rows against the C oracle fed
  the oracle's own pre-processed patterns (1e-5), the <= 1-grey-level contract of the
  pre-processed patterns, and the end-to-end score difference reported.

Reference pipeline: signals/ebsd.py:442-696, pattern/_pattern.py:392-509,
filters/fft_barnes.py:119-177, benchmarks/indexing/test_dictionary_indexing.py:30-63.
"""

import numpy as np
import pytest

import _prep_cases as P
from oracle import c_oracle
from oracle import kpdi_oracle as ko

pytestmark = pytest.mark.gpu
ATOL = 1e-5  # north_star: scores within 1e-5 of the reference


def close_u8(out, ref, max_frac=1e-3):
    """<= 1 grey level on <= 1e-3 of the pixels."""
    d = np.abs(out.astype(np.int64) - ref.astype(np.int64))
    assert d.max() <= 1, f"max grey-level difference {d.max()}"
    assert (d != 0).mean() <= max_frac, f"{(d != 0).mean():.2e} of pixels differ"
    return float((d != 0).mean())


def grey_levels(out, want, dtype):
    """uint8: <= 1 grey level on <= 2e-3 of the pixels (synthetic noise patterns flip a little more
    often than the Ni patterns' 1e-3).  uint16: the reference's float32 FFT round-off (~1e-6 of the
    value) is a sizeable fraction of one of the 65 535 levels, so many pixels differ - by a few levels
    at most, i.e. < 1/16 of a uint8 grey level."""
    d = np.abs(out.astype(np.int64) - want.astype(np.int64))
    if np.dtype(dtype) == np.uint16:
        assert d.max() <= 16, d.max()
    else:
        assert d.max() <= 1 and (d != 0).mean() <= 2e-3, (d.max(), (d != 0).mean())


def codes():
    from kikuchipy_amd import _lib

    return _lib


def run_pipeline(ctx, exp, bg, dic, *, fused, metric="ncc", keep_n=10, mask=None, nav=None, static=True,
                 dynamic=True, scale_bg=False, op="subtract", domain="frequency", compute=None):
    """set_experimental -> (static) -> (dynamic) -> dictionary -> best-k.  `fused=False` reads the
    patterns back after every step, which makes every step run on its own."""
    L = codes()
    sy, sx = exp.shape[-2:]
    ctx.set_problem(sy, sx, mask, {"ncc": L.METRIC_NCC, "ndp": L.METRIC_NDP}[metric], keep_n,
                    L.COMPUTE_F32 if compute is None else compute)
    ctx.set_experimental(exp, nav)
    opc = {"subtract": L.OP_SUBTRACT, "divide": L.OP_DIVIDE}[op]
    steps = []
    if static:
        ctx.remove_static_background(bg.astype(np.float32), opc, scale_bg)
        if not fused:
            steps.append(ctx.get_experimental())
    if dynamic:
        ctx.remove_dynamic_background(opc, {"frequency": L.DOMAIN_FREQUENCY, "spatial": L.DOMAIN_SPATIAL}[domain], 0.0, 4.0)
        if not fused:
            steps.append(ctx.get_experimental())
    ctx.set_profiling(True)
    ctx.reset_counters()
    ctx.push_dictionary_chunk(dic, 0)
    s, i = ctx.finalize(keep_n)
    cnt = ctx.counters()
    ctx.set_profiling(False)
    return s, i, ctx.get_experimental(), steps, cnt


@pytest.fixture(scope="module")
def ctx():
    with codes().Context(0) as c:
        yield c


@pytest.mark.parametrize("dtype,shape,masked,navmask,metric,kw", [
    (np.uint8, (60, 60), True, False, "ncc", {}),
    (np.uint8, (60, 60), False, True, "ndp", {}),
    (np.uint8, (60, 60), True, True, "ncc", dict(scale_bg=True)),
    (np.uint8, (60, 60), False, False, "ncc", dict(op="divide")),
    (np.uint8, (60, 60), True, False, "ncc", dict(domain="spatial")),
    (np.uint8, (60, 60), True, False, "ncc", dict(static=False)),
    (np.uint8, (60, 60), True, False, "ndp", dict(dynamic=False)),
    (np.uint8, (47, 61), True, False, "ncc", {}),          # odd pixel count: scalar loads / stores
    (np.uint16, (60, 60), True, False, "ncc", {}),
    (np.float32, (60, 60), False, False, "ncc", {}),
    (np.uint8, (120, 120), True, False, "ncc", {}),         # 14 400 px: the 64-value register form
    (np.uint8, (136, 140), False, False, "ndp", {}),        # 19 040 px: fused pre-processing, separate preparation
] + [
    # the fused preparation epilogue under the other compute forms (H16 on / off, pix_map, out_row with -1 rows)
    (np.uint8, shape, masked, navmask, "ncc", dict(compute=compute))
    for compute in ("f16", "f16x2", "wide")
    for shape, masked, navmask in (((60, 60), True, True),       # 16 values per thread, pix_map and -1 rows together
                                   ((86, 120), False, False),    # 1024 threads
                                   ((120, 120), True, False),
                                   ((60, 120), False, False),    # 7200 columns on 256 threads: 64 values per thread
                                   ((136, 140), False, False))   # 19 040 columns on 1024 threads: 32 values per thread
])
def test_fused_equals_stepwise(ctx, dtype, shape, masked, navmask, metric, kw, monkeypatch):
    kw = dict(kw)
    compute = kw.pop("compute", None)
    if compute is not None:
        # KPDI_F32_WIDE is read by set_problem: a fresh context per setting (tests/test_gpu_prep_matrix.py)
        monkeypatch.setenv("KPDI_F32_WIDE", "1" if compute == "wide" else "0")
        L = codes()
        with L.Context(0) as fresh:
            fused_equals_stepwise(fresh, dtype, shape, masked, navmask, metric, kw, compute,
                                  {"f16": L.COMPUTE_F16, "f16x2": L.COMPUTE_F16X2, "wide": L.COMPUTE_F32}[compute])
        return
    fused_equals_stepwise(ctx, dtype, shape, masked, navmask, metric, kw, None, None)


def float64_topk(u, dic, mask, metric, keep_n):
    """(scores, indices, form-2 tolerance) of the float64 evaluation of the pre-processed patterns `u` against `dic`; the
    tolerance by the rule of tests/_prep_cases.py: twice the deviation of the same evaluation with its prepared operands
    rounded to float16(2^12 value)."""
    keep = np.arange(u[0].size) if mask is None else np.flatnonzero(~np.asarray(mask).ravel())
    e, d = P.prepared(u, keep, metric), P.prepared(dic, keep, metric)
    exact = e @ d.T
    e16, d16 = ((v * 4096).astype(np.float32).astype(np.float16).astype(np.float64) for v in (e, d))
    tol = 2.0 * float(np.abs((e16 @ d16.T) * 2.0 ** -24 - exact).max())
    idx = np.argsort(-exact, axis=1, kind="stable")[:, :keep_n]
    return np.take_along_axis(exact, idx, axis=1), idx, tol


def fused_equals_stepwise(ctx, dtype, shape, masked, navmask, metric, kw, compute_name, compute):
    rng = np.random.default_rng(11)
    m, n = 37, 300
    hi = 65535 if dtype == np.uint16 else 255
    exp = rng.integers(0, hi + 1, (m,) + shape).astype(dtype)
    bg = rng.integers(1, hi + 1, shape).astype(dtype)
    dic = rng.random((n,) + shape, dtype=np.float32)
    mask = ~ko.circular_window(shape).astype(bool) if masked else None
    nav = (rng.random(m) < 0.3) if navmask else None
    s1, i1, u1, steps, cnt1 = run_pipeline(ctx, exp, bg, dic, fused=False, metric=metric, mask=mask, nav=nav, compute=compute, **kw)
    s2, i2, u2, _, cnt2 = run_pipeline(ctx, exp, bg, dic, fused=True, metric=metric, mask=mask, nav=nav, compute=compute, **kw)
    assert np.array_equal(u1, u2)            # pre-processed patterns: bit for bit
    assert np.array_equal(steps[-1], u1)
    assert cnt1["preproc_launches"] == 0 and cnt2["preproc_launches"] == 1
    if compute_name is not None:
        assert cnt1["match_form"] == cnt2["match_form"] == P.FORMS[compute_name]
    kept = u2 if nav is None else u2[~nav]
    if compute_name in ("f16", "f16x2"):
        # the float16 forms: each run against the float64 evaluation of the same pre-processed patterns - the split-f16
        # form within the project's 1e-5, the float16 form within the tolerance its own rounding gives (_prep_cases.py)
        rs, ri, tol16 = float64_topk(kept, dic, mask, metric, 10)
        tol = tol16 if compute_name == "f16" else ATOL
        print(f"{compute_name} {shape}: tolerance {tol:.2e}; stepwise {np.abs(s1 - rs).max():.2e}, fused {np.abs(s2 - rs).max():.2e}")
        ko.assert_topk_parity(s1, i1, rs, ri, atol=tol, tie=2 * tol)
        ko.assert_topk_parity(s2, i2, rs, ri, atol=tol, tie=2 * tol)
    else:
        assert np.array_equal(i1, i2)
        assert np.abs(s1 - s2).max() <= 1e-6      # the two preparation kernels sum in different orders
        # against the oracle fed the engine's own pre-processed patterns
        rs, ri = ko.dictionary_indexing(kept, dic, metric=metric, keep_n=10, signal_mask=mask)
        ko.assert_topk_parity(s2, i2, rs, ri, atol=ATOL)
    # and the pre-processing against the oracle's (<= 1 grey level on <= 1e-3 of pixels; exact for static only)
    want = exp
    if kw.get("static", True):
        want = ko.remove_static_background(want, bg, kw.get("op", "subtract"), kw.get("scale_bg", False))
    if kw.get("dynamic", True):
        want = ko.remove_dynamic_background(want, kw.get("op", "subtract"), kw.get("domain", "frequency"))
    if not kw.get("dynamic", True):
        assert np.array_equal(u2, want)
    elif dtype == np.float32:
        assert np.allclose(u2, want, atol=2e-4)
    else:
        grey_levels(u2, want, dtype)


def test_recorded_steps_follow_the_patterns(ctx):
    """A second static step, a new pattern set and a reshaped problem all behave like the
    step-by-step API: nothing recorded is lost or applied to the wrong patterns."""
    L = codes()
    rng = np.random.default_rng(5)
    exp = rng.integers(0, 256, (9, 60, 60), dtype=np.uint8)
    bg = rng.integers(1, 256, (60, 60), dtype=np.uint8)
    ctx.set_problem(60, 60, None, L.METRIC_NCC, 1)
    ctx.set_experimental(exp)
    ctx.remove_static_background(bg.astype(np.float32), L.OP_SUBTRACT, False)
    ctx.remove_static_background(bg.astype(np.float32), L.OP_DIVIDE, False)   # cannot fuse: first one runs now
    twice = ko.remove_static_background(ko.remove_static_background(exp, bg), bg, "divide")
    assert np.array_equal(ctx.get_experimental(), twice)
    ctx.remove_dynamic_background(L.OP_SUBTRACT, L.DOMAIN_FREQUENCY, 0.0, 4.0)
    ctx.set_experimental(exp)                                                  # recorded step dropped with the old set
    assert np.array_equal(ctx.get_experimental(), exp)
    ctx.remove_dynamic_background(L.OP_SUBTRACT, L.DOMAIN_FREQUENCY, 0.0, 4.0)
    ctx.remove_dynamic_background(L.OP_SUBTRACT, L.DOMAIN_FREQUENCY, 0.0, 4.0)
    want = ko.remove_dynamic_background(ko.remove_dynamic_background(exp))
    close_u8(ctx.get_experimental(), want, max_frac=3e-3)


@pytest.mark.parametrize("shape,dtype", [((480, 480), np.uint8), ((200, 150), np.uint16), ((150, 200), np.uint8)])
def test_large_detectors_preprocess(ctx, shape, dtype):
    """Raw EBSD detectors (480 x 480 and up) exceed the LDS of the fused kernel: streaming kernels."""
    rng = np.random.default_rng(8)
    hi = 65535 if dtype == np.uint16 else 255
    # smooth background + Kikuchi-like bands + noise: a realistic dynamic range for the filter
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    base = np.exp(-(((yy - shape[0] / 2) / shape[0]) ** 2 + ((xx - shape[1] / 2) / shape[1]) ** 2) * 3)
    exp = np.empty((5,) + shape, dtype=dtype)
    for j in range(5):
        band = 0.15 * np.cos((xx * np.cos(j) + yy * np.sin(j)) / 9.0)
        img = (base + band) * (0.6 + 0.08 * rng.random(shape))
        exp[j] = (img / img.max() * hi * 0.95).astype(dtype)
    bg = (base / base.max() * hi * 0.9).astype(dtype) + 1
    dic = rng.random((24,) + shape, dtype=np.float32)
    mask = ~ko.circular_window(shape).astype(bool)
    s, i, u, _, cnt = run_pipeline(ctx, exp, bg, dic, fused=True, mask=mask, keep_n=5)
    want = ko.remove_dynamic_background(ko.remove_static_background(exp, bg))
    grey_levels(u, want, dtype)
    rs, ri = ko.dictionary_indexing(u, dic, keep_n=5, signal_mask=mask)
    ko.assert_topk_parity(s, i, rs, ri, atol=ATOL)
    # static only is exact at any size
    L = codes()
    ctx.set_experimental(exp)
    ctx.remove_static_background(bg.astype(np.float32), L.OP_SUBTRACT, True)
    assert np.array_equal(ctx.get_experimental(), ko.remove_static_background(exp, bg, "subtract", True))


def test_config3_full(ctx):
    """configs[2] as stated: 4096 x 100 000, circular mask, static + dynamic subtract, ncc, keep_n = 20
    (SURVEY.md 8(d) generator; the reference's benchmarks/indexing/test_dictionary_indexing.py:30-63 chain)."""
    rng = np.random.default_rng(2024)
    exp = rng.integers(0, 256, (4096, 60, 60), dtype=np.uint8)
    dic = rng.random((100000, 60, 60), dtype=np.float32)
    bg = rng.integers(1, 256, (60, 60), dtype=np.uint8)
    mask = ~ko.circular_window((60, 60)).astype(bool)
    assert int((~mask).sum()) == 2819
    s, i, u, _, cnt = run_pipeline(ctx, exp, bg, dic, fused=True, mask=mask, keep_n=20)
    assert cnt["preproc_launches"] == 1 and cnt["k_kept"] == 2819
    rows = np.sort(np.random.default_rng(3).choice(4096, 320, replace=False))
    # (1) the pre-processed patterns against the oracle's: <= 1 grey level on <= 1e-3 of the pixels
    want = ko.remove_dynamic_background(ko.remove_static_background(exp[rows], bg))
    frac = close_u8(u[rows], want)
    # (2) match stage fed the ORACLE's pre-processed patterns: 1e-5 on all 320 rows
    L = codes()
    ctx.set_problem(60, 60, mask, L.METRIC_NCC, 20)
    ctx.set_experimental(want)
    ctx.push_dictionary_chunk(dic, 0)
    s_o, i_o = ctx.finalize(20)
    rs, ri = c_oracle.rows_topk_f64(want, dic, np.arange(len(rows)), "ncc", 20, mask)
    ko.assert_topk_parity(s_o, i_o, rs, ri, atol=ATOL)
    # (3) end to end from the raw patterns: identical wherever the pre-processed rows agree,
    # and within the cost of a flipped grey level elsewhere (~1.6e-5 each)
    same = np.all(u[rows] == want, axis=(1, 2))
    assert same.mean() > 0.5
    ko.assert_topk_parity(s[rows][same], i[rows][same], rs[same], ri[same], atol=ATOL)
    end_to_end = float(np.abs(s[rows] - rs).max())
    assert end_to_end < 1e-4
    assert np.mean(i[rows][:, 0] == ri[:, 0]) > 0.99
    print(f"config3: {frac:.2e} of sampled pixels differ by one grey level; rows identical {same.mean():.3f}; "
          f"end-to-end max |dscore| {end_to_end:.2e}; pre-kernel {cnt['preproc_ms']:.3f} ms")
