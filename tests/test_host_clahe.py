"""Adaptive histogram equalization without a GPU: the host restatement (tests/_clahe_restate.py) pinned bit for bit to
tests/golden/clahe.npz (made by the reference, tools/gen_clahe_golden.py), the clip loop on hand-made histograms, the
reflection, argument handling, error types and texts and warnings (all before any GPU work), how the new callables
bind, and the kernel path choice of csrc/clahe_plan.h compiled with the host compiler."""

import inspect
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import _clahe_cases as cases
import _clahe_restate as R
import _iq_inputs
import kikuchipy_amd as kpa
from conftest import GOLDEN, ROOT
from kikuchipy_amd.pattern import adaptive_histogram_equalization, adaptive_histogram_equalization_stack
from kikuchipy_amd.pattern._pattern import clahe_arguments, clahe_kernel_size

G = np.load(os.path.join(GOLDEN, "clahe.npz"))
PRE = np.load(os.path.join(GOLDEN, "preproc.npz"))


def _inputs():
    yield "ni", PRE["ni"]
    yield "ni_corrected", PRE["ni__static_then_dynamic"]
    for d in cases.DTYPES:
        seed = int(G[f"rand__60x60__{d}__seed"])
        yield f"rand__60x60__{d}", cases.as_dtype(_iq_inputs.stack((60, 60), cases.base_dtype(d), seed), d)
        yield f"degenerate__{d}", cases.degenerate(d)
    for shape in ((61, 59), (59, 61)):
        key = f"rand__{shape[0]}x{shape[1]}__uint8"
        yield key, _iq_inputs.stack(shape, "uint8", int(G[key + "__seed"]))


def fixture_items():
    """(input key, case name, the input's patterns (n, sy, sx), the expected first rows)."""
    for key, stack in _inputs():
        flat = stack.reshape((-1,) + stack.shape[-2:])
        for k in G.files:
            if k.startswith(key + "__") and k.count("__") == key.count("__") + 1 and not k.endswith("__seed"):
                yield key, k[len(key) + 2:], flat, G[k]


def test_fixture_covers_every_case():
    items = list(fixture_items())
    stored = [k for k in G.files if "__" in k and not k.endswith("__seed") and not k.startswith(("error__", "nbins_"))]
    assert len(items) == len(stored)
    assert "numpy 1.26" in str(G["made_by"]) and "skimage 0.18.3" in str(G["made_by"])
    assert {n for key, n, _, _ in items if key == "ni"} == set(cases.NI_CASES)
    used = {cases.args(n) for _, n, _, _ in items}
    assert {k for k, _, _ in used} == {None, 10, (7, 13), (1, 1), (80, 80)}
    assert {c for _, c, _ in used} == set(cases.CLIPS.values())
    assert {b for _, _, b in used} == set(cases.NBINS.values())
    assert {want.dtype.name for _, _, _, want in items} == set(cases.DTYPES)
    assert {flat.shape[-2:] for _, _, flat, _ in items} >= {(60, 60), (61, 59), (59, 61), (32, 32)}
    assert set(cases.ERRORS) == {k[len("error__"):] for k in G.files if k.startswith("error__")}
    assert bool(G["nbins_20000_differs_from_16384"])
    assert os.path.getsize(os.path.join(GOLDEN, "clahe.npz")) < 1 << 20


def test_restatement_matches_the_reference():
    n = 0
    for key, name, flat, want in fixture_items():
        kernel, clip, nbins = cases.args(name)
        got = R.ebsd_equalize(flat[: len(want)], kernel, clip, nbins)
        assert got.dtype == want.dtype, (key, name)
        np.testing.assert_array_equal(got, want, err_msg=f"{key} {name}")
        n += 1
    assert n > 90


def test_reference_facts():
    """What the fixture shows: the default kernel is transposed for non-square patterns, a float32 pattern holding a
    NaN gives a finite result, an all-NaN one (constant after img_as_uint) NaN, a constant uint8 one 0."""
    assert R.ebsd_kernel(None, (61, 59)) == (14, 15) and R.ebsd_kernel(None, (59, 61)) == (15, 14)
    nan = G[f"degenerate__float32__{cases.case('none', 'c0', 'b128')}"]
    assert np.isfinite(nan[1]).all() and np.isnan(nan[4]).all()
    const = G[f"degenerate__uint8__{cases.case('none', 'c0', 'b128')}"]
    # a constant 32 x 32 pattern equalizes to a constant: kikuchipy's rescale is 0 / 0, cast to 0
    assert const.dtype == np.uint8 and const[2].max() == 0 and const[3].max() == 0


def test_clip_histogram_by_hand():
    # nothing over the limit: unchanged
    np.testing.assert_array_equal(R.clip_histogram([1, 2, 3, 0], 5), [1, 2, 3, 0])
    # 10 over on 4 bins: 2 to each bin under the limit, the rest one by one from index 0
    h = R.clip_histogram([20, 0, 0, 0], 10)
    assert h.sum() == 20 and h.max() <= 10
    np.testing.assert_array_equal(h, [10, 4, 3, 3])
    # every bin at the limit: the excess is dropped
    np.testing.assert_array_equal(R.clip_histogram([5, 5, 9], 5), [5, 5, 5])
    # the mid bin (at or above limit - increment after the low bins were raised) is topped up out of the excess; the
    # last 3 go to bins 2 and 3 (step 1), then bin 3 (index 1, step 2)
    np.testing.assert_array_equal(R.clip_histogram([16, 7, 0, 0], 8), [8, 8, 3, 4])
    # limit 1, 2 left for 4 bins under it: step 2 from index 0
    np.testing.assert_array_equal(R.clip_histogram([3, 0, 0, 0, 0], 1), [1, 0, 1, 0, 1])


@pytest.mark.parametrize("n", [1, 2, 5, 60])
def test_reflect_is_numpys(n):
    for k in (1, 2, 7, 15, 80, 200):
        start, end = k // 2, (k - n % k) % k + int(np.ceil(k / 2))
        padded = np.pad(np.arange(n), (start, end), mode="reflect")
        j = np.arange(len(padded)) - start
        got = np.where(j < 0, -1, R.reflect(np.maximum(j, 0), n))
        np.testing.assert_array_equal(got[start:], padded[start:])


def test_reference_errors():
    for name, (dtype, shape, kernel, clip, nbins) in cases.ERRORS.items():
        etype, msg = (str(v) for v in G[f"error__{name}"])
        p = cases.error_input(name)
        with pytest.raises({"ValueError": ValueError, "ZeroDivisionError": ZeroDivisionError}[etype]) as e:
            clahe_arguments(p[None], clahe_kernel_size(kernel, shape), clip, nbins)
        assert str(e.value) == msg, name


def _no_gpu(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("GPU work before the arguments were checked")

    monkeypatch.setattr(kpa.pattern._pattern._lib, "Context", refuse)
    monkeypatch.setattr(kpa.EBSD, "_member_contexts", lambda self, *a: refuse())


def test_argument_handling_before_any_gpu_work(monkeypatch):
    _no_gpu(monkeypatch)
    s = kpa.EBSD(np.zeros((2, 16, 16), np.uint8))
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        s.adaptive_histogram_equalization(lazy_output=True)
    with pytest.raises(ValueError, match=r"Incorrect value of `shape`: \(1, 2, 3\)"):
        s.adaptive_histogram_equalization(kernel_size=(1, 2, 3))
    with pytest.raises(ValueError, match="invalid literal for int"):
        s.adaptive_histogram_equalization(kernel_size=("wrong", "size"))
    with pytest.raises(ZeroDivisionError):
        kpa.EBSD(np.zeros((2, 3, 16), np.uint8)).adaptive_histogram_equalization()  # default kernel (4, 0)
    with pytest.raises(ZeroDivisionError):
        s.adaptive_histogram_equalization(nbins=0)
    with pytest.raises(ValueError, match="'minlength' must not be negative"):
        s.adaptive_histogram_equalization(nbins=-1)
    with pytest.raises(ValueError, match="at most 16384 bins"):
        s.adaptive_histogram_equalization(nbins=16385)
    with pytest.raises(ValueError, match="Images of type float must be between -1 and 1."):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kpa.EBSD(np.full((2, 8, 8), 1.5, np.float32)).adaptive_histogram_equalization()
    with pytest.raises(ValueError, match=r"Incorrect value of `kernel_size`: \[3\]"):
        adaptive_histogram_equalization(np.zeros((8, 8), np.uint8), [3])
    with pytest.raises(ValueError, match="one 2-D pattern"):
        adaptive_histogram_equalization(np.zeros((2, 8, 8), np.uint8), 4)
    with pytest.raises(ValueError, match="index can't contain negative values"):
        adaptive_histogram_equalization_stack(np.zeros((2, 8, 8), np.uint8), (-3, 4))


def test_warnings(monkeypatch):
    _no_gpu(monkeypatch)
    f = np.full((2, 8, 8), 0.5, np.float32)
    with pytest.warns(UserWarning, match="^Equalization of signals with floating point data type has been shown to give "
                                         "bad results. Rescaling intensities to integer intensities is recommended.$"):
        with pytest.raises(ValueError, match="at most 16384"):
            kpa.EBSD(f).adaptive_histogram_equalization(nbins=20000)
    f[0, 1, 1] = np.nan
    with pytest.warns(UserWarning, match="^Equalization of signals with NaN data has been shown to give bad results$"):
        with pytest.raises(ValueError, match="at most 16384"):
            kpa.EBSD(f).adaptive_histogram_equalization(nbins=20000)


def test_kernel_size_and_clip_count():
    assert clahe_kernel_size(None, (60, 60)) == [15, 15]
    assert clahe_kernel_size(None, (61, 59)) == [14, 15]  # HyperSpy's (x, y) taken as (rows, cols)
    assert clahe_kernel_size(10, (60, 60)) == [10, 10] and clahe_kernel_size(7.9, (60, 60)) == [7, 7]
    assert clahe_kernel_size((7, 13.5), (60, 60)) == [7, 13]
    p = np.zeros((1, 60, 60), np.uint8)
    assert clahe_arguments(p, [15, 15], 0, 128) == (15, 15, 225, 128)
    assert clahe_arguments(p, [15, 15], 0.01, 128) == (15, 15, 2, 128)
    assert clahe_arguments(p, [15, 15], 0.001, 128) == (15, 15, 1, 128)
    assert clahe_arguments(p, [15, 15], 1.0, 64) == (15, 15, 225, 64)
    assert clahe_arguments(p, [15, 15], 5.0, 64) == (15, 15, 225, 64)  # above ky * kx clips nothing either
    assert R.clip_count(0.05, 7, 13) == clahe_arguments(p, [7, 13], 0.05, 1)[2] == 4
    # a float pattern holding a NaN skips the range check, as np.min gives NaN
    f = np.full((2, 8, 8), 3.0, np.float32)
    f[:, 0, 0] = np.nan
    assert clahe_arguments(f, [2, 2], 0, 128) == (2, 2, 4, 128)


def _leading(f, n):
    return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[:n]]


def test_signatures_lead_with_the_references_parameters():
    e = inspect.Parameter.empty
    assert _leading(kpa.EBSD.adaptive_histogram_equalization, 7) == [
        ("self", e), ("kernel_size", None), ("clip_limit", 0.0), ("nbins", 128), ("show_progressbar", None),
        ("inplace", True), ("lazy_output", None)]
    assert _leading(adaptive_histogram_equalization, 4) == [("pattern", e), ("kernel_size", e),
                                                            ("clip_limit", 0), ("nbins", 128)]
    assert _leading(adaptive_histogram_equalization_stack, 4) == [("patterns", e), ("kernel_size", None),
                                                                  ("clip_limit", 0), ("nbins", 128)]
    for f, n in ((kpa.EBSD.adaptive_histogram_equalization, 7), (adaptive_histogram_equalization, 4),
                 (adaptive_histogram_equalization_stack, 4)):
        extra = list(inspect.signature(f).parameters.values())[n:]
        assert extra and all(p.kind == p.KEYWORD_ONLY for p in extra), f
    assert "devices" in inspect.signature(kpa.EBSD.adaptive_histogram_equalization).parameters


PLAN_PROBE = r"""
#include "clahe_plan.h"
#include <cstdio>
int main() {
  int sizes[][2] = {{60, 60}, {61, 59}, {1, 64}, {64, 1}, {128, 96}, {240, 240}, {1024, 1024}, {1001, 1001}};
  int kernels[][2] = {{15, 15}, {1, 1}, {2, 2}, {7, 13}, {80, 80}, {256, 256}, {10, 10}, {3000, 3000}};
  int nbins[] = {1, 128, 256, 16384};
  for (int d = 0; d < 9; ++d)
    for (auto &s : sizes)
      for (auto &k : kernels)
        for (int b : nbins)
          for (int force = 0; force < 2; ++force) {
            kpdi::ClahePlan p = kpdi::clahe_plan(d, s[0], s[1], k[0], k[1], b, 262144, force);
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %zu %zu %lld %zu\n", d, s[0], s[1], k[0], k[1], b, force, p.path,
                        p.nty, p.ntx, p.band, p.lds_bytes, p.slot_bytes, (long long)p.per_launch, p.workspace_bytes);
          }
  std::printf("bad %d %d %d %d\n", kpdi::clahe_plan(0, 60, 60, 0, 15, 128, 1).path,
              kpdi::clahe_plan(0, 60, 60, 15, 15, 0, 1).path, kpdi::clahe_plan(0, 60, 60, 15, 15, 16385, 1).path,
              kpdi::clahe_plan(0, 60, 60, 15, 15, 128, 0).path);
}
"""


def test_path_choice(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[-2] == "bad -1 -1 -1 -1"
    es = {0: 1, 1: 2, 2: 4, 3: 8, 4: 1, 5: 2}
    plans = {}
    for line in lines[:-2]:
        d, sy, sx, ky, kx, nb, force, path, nty, ntx, band, lds, slot, per, ws = map(int, line.split())
        plans[(d, sy, sx, ky, kx, nb, force)] = path
        if d not in es:
            assert path == -1
            continue
        if path == -1:
            continue
        assert nty == -(-sy // ky) and ntx == -(-sx // kx) and 1 <= band <= nty
        tables = -(-(sy + sx) * 12 // 16) * 16 + -(-(nty * ky + ntx * kx) * 8 // 16) * 16
        if path == 0:
            assert not force and band == nty and lds <= 64 * 1024
            assert lds == tables + sum(-(-b // 16) * 16 for b in (sy * sx * 2, nty * ntx * nb * 4, nty * ntx * nb * 2))
        else:
            assert lds == tables <= 128 * 1024 and 1 <= per <= 4096 and ws == slot * per <= 512 << 20
            if force and plans[(d, sy, sx, ky, kx, nb, 0)] == 0 and nty > 1:
                assert band < nty  # the band loop runs more than once
    for d in es:  # the issue's minimum coverage, in every dtype
        assert plans[(d, 60, 60, 15, 15, 128, 0)] == 0
        assert plans[(d, 240, 240, 1, 1, 128, 0)] in (0, 1)
        assert plans[(d, 1024, 1024, 256, 256, 128, 0)] == 1 and plans[(d, 1024, 1024, 2, 2, 128, 0)] == 1
        assert plans[(d, 60, 60, 80, 80, 128, 0)] == 0
        for sy, sx in ((60, 60), (61, 59), (240, 240), (1024, 1024), (1001, 1001)):
            for k in ((15, 15), (1, 1), (2, 2), (7, 13), (80, 80), (256, 256), (10, 10)):
                for nb in (1, 128, 256, 16384):
                    assert plans[(d, sy, sx, k[0], k[1], nb, 0)] >= 0, (d, sy, sx, k, nb)
                    assert plans[(d, sy, sx, k[0], k[1], nb, 1)] == 1, (d, sy, sx, k, nb)
    # two workgroups per CU at the defaults
    assert plans[(0, 60, 60, 15, 15, 128, 0)] == 0
