"""Intensity rescaling and normalization without a GPU: the host restatement (tests/_intensity_restate.py) pinned to
tests/golden/intensity.npz (made by the reference, tools/gen_intensity_golden.py) and to the reference's known answers,
numpy 1.26's percentile steps, the integer cast rule, argument errors, how the new callables bind, and the kernel path
choice of csrc/intensity_plan.h compiled with the host compiler."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import _intensity_cases as cases
import _intensity_restate as R
import _iq_inputs
import kikuchipy_amd as kpa
from conftest import GOLDEN, ROOT
from kikuchipy_amd.pattern import (normalize_intensity, normalize_intensity_stack, rescale_intensity,
                                   rescale_intensity_stack)
from kikuchipy_amd.pattern._pattern import DTYPE_RANGE, intensity_dtype_out

G = np.load(os.path.join(GOLDEN, "intensity.npz"))
PRE = np.load(os.path.join(GOLDEN, "preproc.npz"))
DUMMY = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]


def _known(test, names):
    rows, i = [], 0
    while f"known__{test}__{i}__{names[0]}" in G:
        row = []
        for n in names:
            v = G[f"known__{test}__{i}__{n}"]
            if v.dtype.kind == "U":
                v = None if str(v) == "None" else np.dtype(str(v)).type
            elif v.ndim == 0:
                v = v.item()
            row.append(v)
        rows.append(tuple(row))
        i += 1
    return rows


KNOWN_RESCALE = _known("test_rescale_intensity", ["relative", "dtype_out", "answer"])
KNOWN_PERCENTILES = _known("test_rescale_intensity_percentiles", ["percentiles", "answer"])
KNOWN_NORMALIZE = _known("test_normalize_intensity", ["num_std", "divide_by_square_root", "dtype_out", "answer"])


def _inputs():
    yield "ni", PRE["ni"]
    yield "ni_corrected", PRE["ni__static_then_dynamic"]
    for d in cases.DTYPES:
        yield f"dummy__{d}", cases.as_dtype(DUMMY, d)
        yield f"degenerate__{d}", cases.degenerate(d)
    for k in sorted(G.files):
        if k.startswith("rand__") and k.endswith("__seed"):
            key = k[: -len("__seed")]
            shape = tuple(int(v) for v in key.split("__")[1].split("x"))
            dtype = key.split("__")[2]
            yield key, cases.as_dtype(_iq_inputs.stack(shape, str(G[key + "__base"]), int(G[k])), dtype)


def fixture_items():
    """(input key, 'rescale' / 'normalize', case name, the input's patterns (n, sy, sx), the expected first rows)."""
    for key, stack in _inputs():
        flat = stack.reshape((-1,) + stack.shape[-2:])
        for kind, table in (("rescale", cases.RESCALE), ("normalize", cases.NORMALIZE)):
            for name in table:
                k = f"{key}__{kind}__{name}"
                if k in G:
                    yield key, kind, name, flat, G[k]


def test_fixture_covers_every_option_and_dtype():
    items = list(fixture_items())
    assert len(items) > 300 and "numpy 1.26" in str(G["made_by"])
    ni = {(kind, name) for key, kind, name, _, _ in items if key == "ni"}
    assert ni == {("rescale", n) for n in cases.RESCALE} | {("normalize", n) for n in cases.NORMALIZE}
    assert {key.split("__")[1] for key, *_ in items if key.startswith("dummy__")} == set(cases.DTYPES)
    assert os.path.getsize(os.path.join(GOLDEN, "intensity.npz")) < 1 << 20


def test_restatement_matches_the_reference():
    """Rescale bit for bit, except int8 / int16 entries where the reference's integer arithmetic wraps: those match a
    wrapping restatement, and the exact restatement differs.  Normalize within 1e-12 relative (integer input to
    float64), else 2e-5, integer outputs within one level."""
    n_wrapped = 0
    for key, kind, name, flat, want in fixture_items():
        if kind == "rescale":
            args = cases.RESCALE[name]
            got = R.ebsd_rescale(flat, **args)[: len(want)]
            if got.dtype == want.dtype and np.array_equal(got, want, equal_nan=want.dtype.kind == "f"):
                continue
            assert flat.dtype in (np.int8, np.int16), (key, name)
            wrapped = R.ebsd_rescale(flat, wrap=True, **args)[: len(want)]
            np.testing.assert_array_equal(wrapped, want, err_msg=f"{key} {name}")
            n_wrapped += 1
            continue
        got = R.ebsd_normalize(flat, **cases.NORMALIZE[name])[: len(want)]
        assert got.dtype == want.dtype
        if want.dtype.kind == "f":
            g, w = got.astype(np.float64), want.astype(np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(w)), (key, name)
            fin = np.isfinite(w)
            d = np.abs(g - w)[fin]
            tol = 1e-12 * np.abs(w[fin]) if flat.dtype.kind in "iu" and want.dtype == np.float64 else 2e-5
            assert np.all(d <= np.maximum(tol, 1e-300)), (key, name, d.max())
        else:
            d = np.abs(got.astype(np.int64) - want.astype(np.int64))
            span = 1 << (8 * want.dtype.itemsize)
            assert np.minimum(d, span - d).max() <= 1, (key, name)
    assert n_wrapped > 0


def test_restatement_known_answers():
    for relative, dtype_out, answer in KNOWN_RESCALE:
        got = R.ebsd_rescale(DUMMY.reshape(9, 3, 3), relative=relative, dtype_out=dtype_out)[0]
        assert got.dtype == answer.dtype and np.allclose(got, answer, atol=1e-4)
    for percentiles, answer in KNOWN_PERCENTILES:
        got = R.ebsd_rescale(DUMMY.reshape(9, 3, 3).astype(np.float32), percentiles=tuple(percentiles),
                             dtype_out=np.uint8)[0]
        assert np.allclose(got, answer, atol=2)
    for num_std, div, dtype_out, answer in KNOWN_NORMALIZE:
        data = DUMMY.reshape(9, 3, 3) if dtype_out is not None else DUMMY.reshape(9, 3, 3).astype(np.int16)
        got = R.ebsd_normalize(data, num_std, div, dtype_out)[0]
        assert np.allclose(got, answer, atol=1e-4)
    lo0, hi0, lo, hi = G["known__docstring_relative__ni_minmax"]
    s = R.ebsd_rescale(PRE["ni"].reshape(9, 60, 60), relative=True)
    assert (s.min(), s.max(), s[0].min(), s[0].max()) == (lo0, hi0, lo, hi) == (0, 255, 3, 253)
    assert len(KNOWN_RESCALE) == 4 and len(KNOWN_PERCENTILES) == 2 and len(KNOWN_NORMALIZE) == 4


def test_cast_rule():
    """ndarray.astype on x86-64: truncate to int32 (NaN and out-of-range -> INT32_MIN), keep the low bits."""
    v = np.array([-1.5, 300.7, 70000.0, np.nan, 2.0**40, -0.5, 255.9])
    assert list(R.astype(v, np.uint8)) == [255, 44, 112, 0, 0, 0, 255]
    assert list(R.astype(v, np.int8)) == [-1, 44, 112, 0, 0, 0, -1]
    assert list(R.astype(v, np.uint16)) == [65535, 300, 4464, 0, 0, 0, 255]
    assert list(R.astype(v.astype(np.float32), np.int16)) == [-1, 300, 4464, 0, 0, 0, 255]


@pytest.mark.parametrize("dtype", ["uint8", "int16", "float32", "float64"])
def test_quantile_restatement(dtype):
    """numpy 1.26's linear nanpercentile, step by step, equals the installed NumPy's on the same data."""
    rng = np.random.default_rng(1)
    for n in (1, 2, 7, 3600):
        p = cases.as_dtype(rng.random(n) * 250, dtype)
        if p.dtype.kind == "f" and n > 2:
            p[1] = np.nan
        for q in ((0.5, 99.5), (1, 99), (0, 100), (10, 90), (50, 50)):
            want = np.nanpercentile(p, q)
            assert np.allclose(R.nanpercentile(p, q), want, rtol=1e-15, atol=0), (n, q)


def test_errors_and_dtypes():
    p = np.zeros((2, 8, 8), np.uint8)
    s = kpa.EBSD(p)
    with pytest.raises(ValueError, match="'percentiles' must be None if 'in_range' is not None"):
        s.rescale_intensity(in_range=(1, 254), percentiles=(1, 99))
    with pytest.raises(ValueError, match="'in_range' must be None if 'relative' is True"):
        s.rescale_intensity(in_range=(1, 254), relative=True)
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        s.rescale_intensity(lazy_output=True)
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        s.normalize_intensity(lazy_output=True)
    for bad in (np.float16, np.int32, np.uint32, np.int64, bool):
        with pytest.raises(ValueError, match="uint8, int8, uint16, int16, float32, float64"):
            s.rescale_intensity(dtype_out=bad)
        with pytest.raises(ValueError, match="uint8, int8, uint16, int16, float32, float64"):
            s.normalize_intensity(dtype_out=bad)
        with pytest.raises(ValueError, match="is not supported"):
            rescale_intensity(p[0], dtype_out=bad)
    with pytest.raises(ValueError, match=r"Percentiles must be in the range \[0, 100\]"):
        rescale_intensity_stack(p, percentiles=(1, 101))
    assert intensity_dtype_out(None, np.uint16) == np.uint16
    assert DTYPE_RANGE[np.uint8] == (0, 255) and DTYPE_RANGE[np.float32] == (-1, 1)
    assert DTYPE_RANGE[np.int16] == (-32768, 32767)


def _leading(f, n):
    return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[:n]]


def test_signatures_lead_with_the_references_parameters():
    e = inspect.Parameter.empty
    assert _leading(kpa.EBSD.rescale_intensity, 9) == [
        ("self", e), ("relative", False), ("in_range", None), ("out_range", None), ("dtype_out", None),
        ("percentiles", None), ("show_progressbar", None), ("inplace", True), ("lazy_output", None)]
    assert _leading(kpa.EBSD.normalize_intensity, 7) == [
        ("self", e), ("num_std", 1), ("divide_by_square_root", False), ("dtype_out", None), ("show_progressbar", None),
        ("inplace", True), ("lazy_output", None)]
    assert _leading(rescale_intensity, 5) == [("pattern", e), ("in_range", None), ("out_range", None),
                                              ("dtype_out", None), ("percentiles", None)]
    assert _leading(normalize_intensity, 4) == [("pattern", e), ("num_std", 1), ("divide_by_square_root", False),
                                                ("dtype_out", None)]
    for f, n in ((kpa.EBSD.rescale_intensity, 9), (kpa.EBSD.normalize_intensity, 7), (rescale_intensity, 5),
                 (normalize_intensity, 4), (rescale_intensity_stack, 5), (normalize_intensity_stack, 4)):
        extra = list(inspect.signature(f).parameters.values())[n:]
        assert all(p.kind == p.KEYWORD_ONLY for p in extra), f


PLAN_PROBE = r"""
#include "intensity_plan.h"
#include <cstdio>
int main() {
  int sizes[] = {1, 3, 60, 61, 90, 127, 128, 181, 240, 256, 1001, 1024};
  for (int d = 0; d < 9; ++d)
    for (int sy : sizes)
      for (int sx : sizes) {
        kpdi::IntPlan p = kpdi::int_plan(d, sy, sx, 262144);
        std::printf("%d %d %d %d %zu %d\n", d, sy, sx, p.path, p.lds_bytes, p.select_passes);
      }
  std::printf("bad %d %d\n", kpdi::int_plan(0, 0, 60, 1).path, kpdi::int_plan(0, 60, 60, 0).path);
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
    assert lines[-2] == "bad -1 -1"
    es = {0: 1, 1: 2, 2: 4, 3: 8, 4: 1, 5: 2}
    plans = {}
    for line in lines[:-2]:
        d, sy, sx, path, lds, passes = map(int, line.split())
        plans[(d, sy, sx)] = path
        if d not in es:  # float16 / int32 / uint32 have no path
            assert path == -1
            continue
        staged = (sy * sx * es[d] + 15) // 16 * 16
        assert passes == es[d]
        assert (path == 0) == (staged <= 64 * 1024) and path in (0, 1)
        assert lds == (staged if path == 0 else 0)
    assert plans[(0, 60, 60)] == 0 and plans[(0, 240, 240)] == 0 and plans[(2, 128, 128)] == 0
    assert plans[(3, 90, 90)] == 0 and plans[(3, 128, 128)] == 1
    assert plans[(0, 1024, 1024)] == 1 and plans[(3, 1024, 1024)] == 1
