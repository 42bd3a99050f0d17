"""The PCA decomposition without a GPU: csrc/decomp_plan.h compiled with the host compiler (branch choice, tile and edge
counts of every case of tests/_decomposition_cases.py, the size limit), the NumPy restatement against itself (the model
from the Gram + eigh route that the package takes equals the model from a direct SVD), the `components` forms against
the reference's `_update_learning_results` slicing, the signatures, and the calls that are refused before any GPU
work."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import _decomposition_cases as cases
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.pattern import _decomposition as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAN_PROBE = r"""
#include <cstdio>
#include "decomp_plan.h"
using namespace kpdi;
int main() {
  const long long shapes[][2] = {%s};
  for (auto &s : shapes) {
    const DecPlan p = dec_plan(s[0], s[1]);
    std::printf("%%lld %%lld %%d %%d %%d %%lld %%lld %%d %%d %%lld %%lld %%d\n", s[0], s[1], p.ok, p.too_large, p.transposed,
                (long long)p.side, (long long)p.reduce, p.tiles, p.edge, (long long)p.computed_tiles, (long long)p.steps, p.tail);
  }
  std::printf("const %%d %%d %%d %%d %%lld %%d %%zu\n", DEC_TILE, DEC_KB, DEC_THREADS, DEC_LD, (long long)DEC_MAX_SIDE,
              DEC_MEAN_ROWS, DEC_LDS_BYTES);
  std::printf("chunks %%lld %%lld %%lld\n", (long long)dec_mean_chunks(1), (long long)dec_mean_chunks(256),
              (long long)dec_mean_chunks(257));
  return 0;
}
"""
EXTRA_SHAPES = [(40000, 3600), (8192, 8192), (8193, 8192), (8192, 8193), (8193, 8193), (100000, 8193), (64, 64), (65, 64),
                (1, 1), (16, 5), (17, 5), (1, 7), (0, 5), (5, 0), (-1, 5)]


def test_plan_header(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    shapes = [cases.dims(n) for n in cases.CASES] + EXTRA_SHAPES
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PLAN_PROBE % ", ".join("{%d, %d}" % s for s in shapes))
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert lines[-2] == f"const {cases.TILE} {cases.KB} {cases.THREADS} 80 {cases.MAX_SIDE} {cases.MEAN_ROWS} 20480"
    assert lines[-1] == "chunks 1 1 2"
    assert _lib.DECOMPOSITION_MAX_SIDE == cases.MAX_SIDE
    got = {}
    for line in lines[:-2]:
        m, k, ok, too_large, transposed, side, reduce_, tiles, edge, computed, steps, tail = map(int, line.split())
        got[(m, k)] = dict(ok=ok, too_large=too_large, transposed=transposed, side=side, reduce=reduce_, tiles=tiles,
                           edge=edge, computed_tiles=computed, steps=steps, tail=tail)
    for m, k in shapes:
        g = got[(m, k)]
        if m < 1 or k < 1:
            assert g["ok"] == 0 and g["too_large"] == 0
            continue
        want = cases.plan(m, k)
        assert {n: g[n] for n in want} == want, (m, k)
    # the table's cases: both branches, full and partial tiles, full and partial last stages
    assert (got[cases.dims("A")]["transposed"], got[cases.dims("A")]["tiles"], got[cases.dims("A")]["edge"]) == (0, 2, 27)
    assert (got[cases.dims("B")]["tiles"], got[cases.dims("B")]["edge"], got[cases.dims("B")]["tail"]) == (3, 15, 3)
    assert (got[cases.dims("C")]["transposed"], got[cases.dims("C")]["tiles"], got[cases.dims("C")]["edge"]) == (1, 1, 48)
    assert got[cases.dims("C")]["tail"] == 16 and got[cases.dims("C")]["steps"] == 15
    assert (got[cases.dims("D")]["tiles"], got[cases.dims("D")]["steps"], got[cases.dims("D")]["tail"]) == (1, 132, 4)
    assert (got[cases.dims("E")]["transposed"], got[cases.dims("E")]["side"], got[cases.dims("E")]["steps"]) == (1, 9, 225)
    # the limit is on the SHORTER side
    assert got[(8192, 8192)]["ok"] == 1 and got[(8193, 8192)]["ok"] == 1 and got[(8192, 8193)]["ok"] == 1
    assert got[(8193, 8193)] == dict(got[(8193, 8193)], ok=0, too_large=1) and got[(100000, 8193)]["too_large"] == 1
    assert got[(40000, 3600)]["computed_tiles"] == 57 * 58 // 2


def numpy_results(x, centre, c):
    """The package's own route (`results_from_gram`: eigh of the Gram matrix, the products, the null and sign rules) with
    NumPy in place of the GPU."""
    xc, mean = cases.centred(x, centre)
    g, transposed = cases.gram(xc)
    factors, loadings, variance, ratio = D.results_from_gram(
        g, transposed, lambda basis, t: (xc.T @ basis) if t else (xc @ basis), x.shape[0], c)
    return xc, mean, factors, loadings, variance, ratio


@pytest.mark.parametrize("name", ["A", "C"])
@pytest.mark.parametrize("centre", cases.CENTRES)
def test_gram_route_equals_direct_svd(name, centre):
    x = cases.matrix(cases.low_rank_patterns(name))
    m, k = x.shape
    side = min(m, k)
    xc, mean, factors, loadings, variance, ratio = numpy_results(x, centre, 12)
    f0, l0, v0, s = cases.svd_results(xc, 12)
    lam = s ** 2
    assert variance.shape == (side,) and np.all(np.diff(variance) <= 0) and abs(ratio.sum() - 1) < 1e-12
    assert np.max(np.abs(variance * m - lam)) <= side * 2.0 ** -52 * lam[0]
    err = cases.gram_error(xc)
    for components in (3, 8, [0, 2, 5], None):
        gap = cases.edges_gap(lam, components, 12)
        bound = 2 * err / gap * s[0]
        for dt in (np.float32, np.float64):
            got = cases.model(factors, loadings, mean, centre, components, dt)
            want = cases.model(f0, l0, mean, centre, components, dt)
            ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(got - want) <= bound + ulp), (components, dt)
    gap = min(cases.edges_gap(lam, [j], 12) for j in range(12))
    assert np.max(np.abs(factors - f0)) <= 2 * err / gap * s[0] + 2.0 ** -52
    assert np.max(np.abs(loadings - l0)) <= 2 * err / gap * s[0] + 2.0 ** -52


def test_null_components_are_exactly_zero():
    x = cases.matrix(cases.patterns("C", np.float32))
    xc, mean, factors, loadings, variance, _ = numpy_results(x, "navigation", 48)  # rank <= 47
    assert not factors[:, 47].any() and not loadings[:, 47].any()
    assert factors[:, :40].any(axis=0).all()
    f0, l0, _, _ = cases.svd_results(xc, 48)
    assert not f0[:, 47].any() and not l0[:, 47].any()


def test_sign_rule_and_first_maximum_on_a_tie():
    f = np.array([[1.0, -2.0, 0.5], [-3.0, 2.0, -0.5], [3.0, 1.0, 0.25]])
    lo = np.ones((2, 3))
    g, h = f.copy(), lo.copy()
    D.fix_signs(g, h)
    f2, l2 = f.copy(), lo.copy()
    cases.sign_rule(f2, l2)
    assert np.array_equal(g, f2) and np.array_equal(h, l2)
    assert np.array_equal(g[:, 0], [-1.0, 3.0, -3.0])  # |-3| == |3|: the first, negative one decides
    assert np.array_equal(g[:, 1], [2.0, -2.0, -1.0]) and np.array_equal(g[:, 2], f[:, 2])
    assert np.array_equal(h, [[-1.0, -1.0, 1.0]] * 2)


def test_components_forms_follow_update_learning_results():
    rng = np.random.default_rng(5)
    lr = D.LearningResults(rng.standard_normal((6, 5)), rng.standard_normal((4, 5)), data_shape=(4, 2, 3))
    for components, cols in ((None, [0, 1, 2, 3, 4]), (3, [0, 1, 2]), (5, [0, 1, 2, 3, 4]), (9, [0, 1, 2, 3, 4]),
                             ([0, 2, 4], [0, 2, 4]), ([3, 1], [3, 1]), (np.array([4]), [4])):
        for dt in ("float32", np.float64):
            f, lo = D.select_components(lr, components, dt)
            assert f.dtype == np.dtype(dt) and lo.dtype == np.dtype(dt)
            assert np.array_equal(f, lr.factors.astype(dt)[:, cols]) and np.array_equal(lo, lr.loadings.astype(dt)[:, cols])
            assert np.array_equal(cases.pick(lr.factors, components), lr.factors[:, cols])
    assert lr.factors.dtype == np.float64  # the results themselves stay as they are
    with pytest.raises(ValueError, match="selects no component"):
        D.check_model((4, 2, 3), lr, 0, "float32")
    with pytest.raises(ValueError, match="float32 or float64"):
        D.check_model((4, 2, 3), lr, None, "float16")
    with pytest.raises(ValueError, match=r"shape \(4, 3, 2\) do not match"):
        D.check_model((4, 3, 2), lr, None, "float32")


def test_refusals_come_before_any_gpu_work():
    s = kpa.EBSD(np.zeros((3, 4, 6, 5), dtype=np.uint8), static_background=np.ones((6, 5), dtype=np.uint8))
    assert s.learning_results is None
    with pytest.raises(ValueError, match="No learning results"):
        s.get_decomposition_model()
    with pytest.raises(TypeError, match=r"change_dtype\('float32'\)"):
        s.decomposition()
    with pytest.raises(TypeError, match=r"change_dtype\('float32'\)"):
        kpa.pattern.decomposition_stack(s.data)
    f = kpa.EBSD(np.zeros((3, 4, 6, 5), dtype=np.float32))
    for kw, name in ((dict(algorithm="NMF"), "algorithm"), (dict(normalize_poissonian_noise=True), "normalize_poissonian_noise"),
                     (dict(centre="variance"), "centre"), (dict(svd_solver="randomized"), "svd_solver"),
                     (dict(navigation_mask=np.zeros((3, 4), bool)), "navigation_mask"), (dict(reproject="signal"), "reproject")):
        with pytest.raises(NotImplementedError, match=name):
            f.decomposition(**kw)
    for bad in (0, 13, -1, 2.5, True):
        with pytest.raises(ValueError, match="output_dimension"):
            f.decomposition(output_dimension=bad)
    with pytest.raises(ValueError, match="float16 is not supported"):
        s.change_dtype(np.float16)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.float32), (8200, 100, 100), (0, 0, 0))
    with pytest.raises(ValueError, match=r"EBSD\.downsample"):
        kpa.pattern.decomposition_stack(big)
    assert s._ctx is None and f._ctx is None and f.learning_results is None
    # results do not travel with copies, and an in-place downsample forgets them
    f._learning_results = D.LearningResults(np.zeros((30, 2)), np.zeros((12, 2)), data_shape=f.data.shape)
    assert f.deepcopy().learning_results is None and f._like(f.data).learning_results is None
    f.data = np.zeros((3, 4, 6, 6), dtype=np.float32)
    with pytest.raises(ValueError, match="do not match the learning results"):
        f.get_decomposition_model()
    assert f._ctx is None


def test_signatures_are_the_reference_s():
    def params(fn):
        return [(p.name, p.default, p.kind) for p in inspect.signature(fn).parameters.values()][1:]

    pk, ko, vk = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD
    e = inspect.Parameter.empty
    assert params(kpa.EBSD.get_decomposition_model) == [("components", None, pk), ("dtype_out", "float32", pk)]
    assert params(kpa.EBSD.decomposition) == [("normalize_poissonian_noise", False, pk), ("algorithm", "SVD", pk),
                                              ("output_dimension", None, pk), ("centre", None, pk), ("kwargs", e, vk)]
    assert params(kpa.EBSD.change_dtype) == [("dtype", e, pk)]
    assert isinstance(kpa.EBSD.learning_results, property)
    assert [(p.name, p.default, p.kind) for p in inspect.signature(kpa.pattern.decomposition_stack).parameters.values()] == [
        ("patterns", e, pk), ("output_dimension", None, pk), ("centre", None, pk), ("context", None, ko)]
    for name in ("decomposition_gram", "decomposition_apply", "decomposition_model", "change_dtype"):
        assert "kpdi_" + name in _lib.SIGNATURES and callable(getattr(_lib.Context, name))
    assert (_lib.CENTRE_NONE, _lib.CENTRE_NAVIGATION, _lib.CENTRE_SIGNAL) == (0, 1, 2)


def test_means_restatement_is_a_mean():
    x = cases.matrix(cases.patterns("D", np.float32))
    assert np.allclose(cases.mean_signal(x), x.mean(axis=1), rtol=1e-13, atol=0)
    assert np.allclose(cases.mean_navigation(x), x.mean(axis=0), rtol=1e-13, atol=0)
    xi = cases.matrix(cases.integers("A", np.uint16))
    assert np.array_equal(cases.mean_signal(xi), xi.sum(axis=1) / xi.shape[1])  # integer sums are exact in any order
    assert np.array_equal(cases.mean_navigation(xi), xi.sum(axis=0) / xi.shape[0])
