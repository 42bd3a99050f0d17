"""The PCA decomposition on the GPU (csrc/decomp.hip through the C ABI, `kikuchipy_amd.pattern.decomposition_stack` and
the `EBSD` methods) against the float64 NumPy restatement of tests/_decomposition_cases.py.  Every bound is computed by
the test from the restatement: the standard dot-product bound for the products, Davis-Kahan for the end-to-end model.
Every test prints its error / bound ratio before it asserts (run with -s to see them)."""

import numpy as np
import pytest

import _decomposition_cases as cases
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import _decomposition as D
from kikuchipy_amd.pattern import _pattern

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
CODE = D.CENTRES


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def upload(ctx, p):
    _pattern._upload(ctx, p)
    return cases.matrix(p)


# ---- (a) exact Gram -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_gram_of_integers_is_exact(ctx, name, dtype):
    p = cases.integers(name, dtype)
    upload(ctx, p)
    g, mean, transposed = ctx.decomposition_gram(_lib.CENTRE_NONE)
    xi = p.reshape(cases.dims(name)).astype(np.int64)
    want = xi @ xi.T if transposed else xi.T @ xi
    assert transposed == (cases.plan(*cases.dims(name))["transposed"] == 1) and mean is None
    assert np.abs(want).max() < 2 ** 53
    assert g.shape == want.shape and np.array_equal(g, want.astype(np.float64))
    assert np.array_equal(ctx.get_experimental(), p.reshape((-1,) + p.shape[-2:]))  # the patterns are only read


# ---- (b) centred Gram ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("centre", ["navigation", "signal"])
@pytest.mark.parametrize("name", list(cases.CASES))
def test_centred_gram(ctx, name, centre, dtype):
    x = upload(ctx, cases.patterns(name, dtype))
    g, mean, transposed = ctx.decomposition_gram(CODE[centre])
    xc, mu = cases.centred(x, centre)
    assert np.array_equal(mean, mu)  # the documented summation order, bit for bit
    want, t = cases.gram(xc)
    a = np.abs(xc)
    n = xc.shape[1] if t else xc.shape[0]
    bound = 2 * (n + 2) * U * (a @ a.T if t else a.T @ a)
    assert t == transposed and np.array_equal(g, g.T)
    ratio = float(np.max(np.abs(g - want) / bound))
    print(f"centred gram {name} {centre} {np.dtype(dtype).name}: max error / bound = {ratio:.3g}")
    assert ratio <= 1.0


# ---- (c) apply ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centre", cases.CENTRES)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_apply(ctx, name, centre):
    x = upload(ctx, cases.patterns(name, np.float32))
    xc, _ = cases.centred(x, centre)
    m, k = x.shape
    rng = np.random.default_rng(m + k)
    for c in (1, 5, min(m, k)):
        for transposed_op, op in ((False, xc), (True, xc.T)):
            basis = rng.standard_normal((op.shape[1], c))
            got = ctx.decomposition_apply(basis, CODE[centre], transposed_op)
            bound = 2 * (op.shape[1] + 2) * U * (np.abs(op) @ np.abs(basis))
            ratio = float(np.max(np.abs(got - op @ basis) / bound))
            print(f"apply {name} {centre} c={c} transposed_op={transposed_op}: max error / bound = {ratio:.3g}")
            assert got.shape == (op.shape[0], c) and ratio <= 1.0


# ---- (d) model arithmetic -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_out", [np.float32, np.float64])
@pytest.mark.parametrize("centre", cases.CENTRES)
@pytest.mark.parametrize("name", ["A", "B", "C", "E"])
def test_model_arithmetic(ctx, name, centre, dtype_out):
    m, k = cases.dims(name)
    rng = np.random.default_rng(m * k)
    upload(ctx, cases.integers(name, np.uint8))
    for c in (1, 7, min(m, k, 40)):
        lo = rng.standard_normal((m, c)).astype(dtype_out)
        fa = rng.standard_normal((k, c)).astype(dtype_out)
        mean = None if centre is None else 100.0 * rng.standard_normal(m if centre == "signal" else k)
        ctx.decomposition_model(lo, fa, mean, CODE[centre], dtype_out)
        got = ctx.get_experimental().reshape(m, k)
        assert got.dtype == np.dtype(dtype_out)
        want = cases.model(fa, lo, mean, centre, None, dtype_out)
        if dtype_out is np.float32:
            w32 = want.astype(np.float32)
            assert np.all(np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)))
        else:
            mag = np.abs(lo.astype(np.float64)) @ np.abs(fa.astype(np.float64)).T
            if centre is not None:
                mag = mag + (np.abs(mean)[:, None] if centre == "signal" else np.abs(mean)[None, :])
            ratio = float(np.max(np.abs(got - want) / (2 * (c + 2) * U * mag)))
            print(f"model {name} {centre} c={c}: max error / bound = {ratio:.3g}")
            assert ratio <= 1.0
        upload(ctx, cases.integers(name, np.uint8))  # the next round replaces patterns of another dtype again


# ---- (e) end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,centre", [("A", None), ("A", "signal"), ("A", "navigation"), ("C", None), ("C", "signal"),
                                         ("C", "navigation")])
def test_end_to_end_through_ebsd(name, centre):
    p = cases.low_rank_patterns(name)
    x = cases.matrix(p)
    m, k = x.shape
    side = min(m, k)
    xc, mean = cases.centred(x, centre)
    f0, l0, v0, sv = cases.svd_results(xc, 12)
    lam = sv ** 2
    err = cases.gram_error(xc)
    with kpa.EBSD(p, device=0) as s:
        s.decomposition(output_dimension=12, centre=centre)
        lr = s.learning_results
        assert lr.factors.shape == (k, 12) and lr.loadings.shape == (m, 12) and lr.factors.dtype == np.float64
        assert lr.explained_variance.shape == (side,) and lr.centre == centre and lr.output_dimension == 12
        assert (mean is None and lr.mean is None) or np.array_equal(lr.mean, mean)
        d = float(np.max(np.abs(lr.explained_variance * m - lam)))
        print(f"e2e {name} {centre}: max |M ev - sigma^2| = {d:.3g}, bound {side * 2.0 ** -52 * lam[0]:.3g}")
        assert d <= side * 2.0 ** -52 * lam[0]
        assert np.array_equal(lr.explained_variance_ratio, lr.explained_variance / lr.explained_variance.sum())
        gap = min(cases.edges_gap(lam, [j], 12) for j in range(12))
        bound = 2 * err / gap * sv[0]
        df, dl = float(np.max(np.abs(lr.factors - f0))), float(np.max(np.abs(lr.loadings - l0)))
        print(f"e2e {name} {centre}: factors {df:.3g}, loadings {dl:.3g}, bound {bound:.3g}")
        assert df <= bound + 2.0 ** -52 and dl <= bound + 2.0 ** -52
        before = (lr.factors.copy(), lr.loadings.copy())
        for components in (3, 8, [0, 2, 5]):
            bound = 2 * err / cases.edges_gap(lam, components, 12) * sv[0]
            want = cases.model(f0, l0, mean, centre, components, np.float32)
            sm = s.get_decomposition_model(components=components)
            assert sm.data.dtype == np.float32 and sm.data.shape == p.shape and sm.learning_results is None
            diff = np.abs(sm.data.reshape(m, k).astype(np.float64) - want)
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            print(f"e2e {name} {centre} components={components}: max error {diff.max():.3g}, Davis-Kahan part {bound:.3g}, "
                  f"max (error - ulp) / bound = {float(np.max((diff - ulp) / bound)):.3g}")
            assert np.all(diff <= bound + ulp)
        assert s.learning_results is lr and np.array_equal(lr.factors, before[0]) and np.array_equal(lr.loadings, before[1])


def test_null_components_are_exactly_zero():
    p = cases.patterns("C", np.float32)
    lr = kpa.pattern.decomposition_stack(p, 48, "navigation")  # 48 patterns minus their mean: rank <= 47
    assert not lr.factors[:, 47].any() and not lr.loadings[:, 47].any()
    assert lr.factors[:, :40].any(axis=0).all() and lr.explained_variance[47] <= 48 * 2.0 ** -52 * lr.explained_variance[0]


# ---- (f) the tutorial's call sequence -----------------------------------------------------------------------------------
def test_tutorial_sequence():
    p = cases.patterns("A", np.uint8)
    bg = p.reshape((-1,) + p.shape[-2:]).mean(axis=0).astype(np.uint8)
    xmap = kpa.signals.DictionaryXmap.empty(p.shape[:2])
    with kpa.EBSD(p.copy(), static_background=bg, xmap=xmap, device=0) as s:
        det = s.detector
        dtype_orig = s.data.dtype
        s.change_dtype("float32")
        assert s.data.dtype == np.float32 and np.array_equal(s.data, p.astype(np.float32))
        s.decomposition(algorithm="SVD", output_dimension=50, centre="signal")
        s.change_dtype(dtype_orig)
        assert s.data.dtype == np.uint8 and np.array_equal(s.data, p)  # the round trip, bit for bit
        assert s.static_background is bg and s.learning_results.factors.shape == (91, 50)
        s2 = s.get_decomposition_model(components=30)
        assert s2.data.dtype == np.float32 and s2.data.shape == p.shape
        assert s2.learning_results is None and s.learning_results is not None
        assert s2.static_background is bg and s2.xmap is xmap and s2.detector.shape == det.shape and s2.detector is not det
        with s2:
            iq = s2.get_image_quality()
            assert iq.shape == p.shape[:2] and np.isfinite(iq).all()
        # 30 of 91 components of noisy patterns: the model is close to, and not the same as, the patterns
        rel = np.linalg.norm(s2.data - p) / np.linalg.norm(p - p.mean())
        assert 0 < rel < 1


@pytest.mark.parametrize("src", [np.uint8, np.int8, np.uint16, np.int16, np.float32, np.float64])
def test_change_dtype_is_astype(ctx, src):
    rng = np.random.default_rng(3)
    if np.dtype(src).kind == "f":
        p = (rng.standard_normal((5, 7, 9)) * 3e4).astype(src)
        p[0, 0, :4] = [0.5, -0.5, 255.9, -129.2]
    else:
        info = np.iinfo(src)
        p = rng.integers(info.min, int(info.max) + 1, (5, 7, 9)).astype(src)
    for dst in (np.uint8, np.int8, np.uint16, np.int16, np.float32, np.float64):
        _pattern._upload(ctx, p)
        ctx.change_dtype(dst)
        got = ctx.get_experimental()
        with np.errstate(invalid="ignore"):
            want = p.astype(dst) if np.dtype(src).kind != "f" or np.dtype(dst).kind == "f" else \
                p.astype(np.int32).astype(dst)  # the documented cast: truncate to int32, keep the low bits
        assert got.dtype == np.dtype(dst) and np.array_equal(got, want), (src, dst)


# ---- (g) repeatability --------------------------------------------------------------------------------------------------
def test_repeatable_and_patterns_untouched():
    p = cases.low_rank_patterns("B")
    keep = p.copy()
    with kpa.EBSD(p, device=0) as s:
        runs = []
        for _ in range(2):
            s.decomposition(output_dimension=20, centre="navigation")
            lr = s.learning_results
            runs.append((lr.factors, lr.loadings, lr.explained_variance, lr.mean))
        for a, b in zip(*runs):
            assert a is not b and np.array_equal(a, b)
        assert s.data is p and np.array_equal(p, keep)
        _pattern._upload(s.context, p)
        g1 = s.context.decomposition_gram(_lib.CENTRE_SIGNAL)[0]
        assert np.array_equal(s.context.get_experimental().reshape(p.shape), keep)  # the resident patterns too
        assert np.array_equal(g1, s.context.decomposition_gram(_lib.CENTRE_SIGNAL)[0])
        model = s.get_decomposition_model(components=10)
    rng = np.random.default_rng(9)
    dic = rng.random((40,) + p.shape[-2:]).astype(np.float32)
    dic[7] = model.data[3, 4]
    with model, kpa.EBSD(dic, xmap=kpa.signals.DictionaryXmap.empty(40), device=0) as dictionary:
        res = model.dictionary_indexing(dictionary, keep_n=3, verbose=False)
    assert np.asarray(res.simulation_indices).reshape(p.shape[:2] + (-1,))[3, 4, 0] == 7


# ---- refused calls ------------------------------------------------------------------------------------------------------
def test_refused_calls_at_the_c_abi(ctx):
    p = cases.patterns("A", np.float32)
    upload(ctx, p)
    m, k = cases.dims("A")
    for call, text in ((lambda: ctx.decomposition_gram(3), "centre 3"),
                       (lambda: ctx.decomposition_apply(np.zeros((k, 92)), 0, False), "92 components"),
                       (lambda: ctx.decomposition_model(np.zeros((m, 2)), np.zeros((k, 2)), np.zeros(5), 2), "mean of 5"),
                       (lambda: ctx.decomposition_model(np.zeros((m, 2)), np.zeros((k, 2)), None, 0, np.uint8), "float32 or float64"),
                       (lambda: ctx.change_dtype(np.float16), "cast to")):
        with pytest.raises(_lib.KpdiError, match=text):
            call()
    bad = p.copy()
    bad[2, 3, 1, 1] = np.nan
    upload(ctx, bad)
    with pytest.raises(_lib.KpdiError, match="patterns hold non-finite values"):
        ctx.decomposition_gram(_lib.CENTRE_NONE)
    ctx.set_problem(100, 100, None, _lib.METRIC_NCC, 1)
    ctx.set_experimental(np.zeros((8200, 100, 100), dtype=np.uint8))
    with pytest.raises(_lib.KpdiError, match="downsample"):
        ctx.decomposition_gram(_lib.CENTRE_NONE)
    assert np.array_equal(ctx.get_experimental()[:2], np.zeros((2, 100, 100), dtype=np.uint8))
