"""Downsampling and the dynamic background without a GPU: the NumPy restatement (tests/_downsample_restate.py) pinned to
the reference's own results (tests/golden/downsample.npz, made by tools/gen_downsample_golden.py), the reference's known
answers, the kernel path choice (csrc/downsample_plan.h compiled with the host compiler), the error messages and
signatures of the mirrored methods, and what `EBSD.downsample` leaves untouched when it refuses.

Contract of the dynamic background (the fixture's `bgdist__*` entries hold the restatement's distance to the reference,
measured when the fixture was made): integer results at most 1 level off on at most 1e-3 of the values - the
restatement differs on at most 8.2e-5 of them (frequency domain) and on none (spatial domain); float results in the
frequency domain within 4.6e-5 to 1.5e-4 on values of 150 to 450, the reference's float32 FFT round-off (bound: twice
that plus 2^-24 max |value|, 1.0e-4 to 3.3e-4); float results in the spatial domain equal, float32 and float64 (bound:
2^-24 max |value|, 0.9e-5 to 2.5e-5)."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import _downsample_cases as cases
import _downsample_restate as R
import kikuchipy_amd as kpa
from kikuchipy_amd.pattern import _pattern

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "downsample.npz"))
INPUTS = cases.inputs()
DUMMY = np.load(os.path.join(ROOT, "tests", "golden", "di_dummy.npz"))["dummy"]
INT_SHARE_CAP = 1e-3  # the project's standing contract for the dynamic background: <= 1 level on <= 1e-3 of the values


def float_bound(k):
    """What a float background may differ from the fixture by: twice the restatement's measured distance to the
    reference plus the float32 rounding of the result, 2^-24 max |value| - both sides are then within one such distance
    of the exact blur."""
    d, vmax = G["bgdist__" + k]
    return 2.0 * d + 2.0 ** -24 * vmax


def check_background(got, k):
    """`got` (the first patterns of a case) against the fixture entry `k`: (share of differing values, max levels) for
    integer results, (max |difference|, bound) for float ones - after asserting the contract."""
    want = G[k]
    got = got[: len(want)]
    assert got.dtype == want.dtype and got.shape == want.shape, k
    if want.dtype.kind == "f":
        d = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
        assert d <= float_bound(k), (k, d, float_bound(k))
        return d, float_bound(k)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    share, levels = float(np.mean(diff != 0)), int(diff.max())
    assert levels <= 1 and share <= INT_SHARE_CAP, (k, share, levels)
    return share, levels


def test_fixture_was_made_by_the_reference():
    made_by = str(G["made_by"])
    assert "reference" in made_by and "numpy 1.26" in made_by and "scipy" in made_by
    assert len(cases.downsample_cases()) == len({cases.key("ds", *c) for c in cases.downsample_cases()})
    for c in cases.downsample_cases():
        assert cases.key("ds", *c) in G.files
    for c in cases.background_cases():
        assert cases.key("bg", *c) in G.files and "bgdist__" + cases.key("bg", *c) in G.files


def test_restatement_of_downsample_is_bit_exact():
    seen = set()
    for name, factor, dtype_out in cases.downsample_cases():
        k = cases.key("ds", name, factor, dtype_out)
        want = G[k]
        stack = INPUTS[name][: cases.stored(name)]
        got = R.downsample_stack(stack, factor, dtype_out)
        assert got.dtype == want.dtype and got.shape == want.shape, k
        assert got.shape[-2:] == (stack.shape[-2] // factor, stack.shape[-1] // factor)
        assert np.array_equal(got, want, equal_nan=want.dtype.kind == "f"), k
        seen.add((stack.dtype.name, want.dtype.name))
    assert len(seen) >= 24  # input x output dtypes covered
    # the special cases say what the reference does: NaN anywhere and a constant binned image are NaN / 0
    f = G[cases.key("ds", "special__float32", 2, "float32")]
    assert np.isfinite(f[0]).all() and np.isnan(f[1]).all() and np.isnan(f[2]).all()
    u = G[cases.key("ds", "special__float32", 2, "uint8")]
    assert u[0].max() == 255 and not u[1].any() and not u[2].any()
    assert not G[cases.key("ds", "dummy__uint8", 3, None)].any()  # 3 x 3 -> 1 x 1: constant


def test_restatement_of_the_background_is_inside_the_contract():
    worst_share = 0.0
    for name, case, dtype_out in cases.background_cases():
        k = cases.key("bg", name, case, dtype_out)
        got = R.get_dynamic_background(INPUTS[name], dtype_out=dtype_out, **cases.BACKGROUND[case])
        a, b = check_background(got, k)
        if G[k].dtype.kind != "f":
            worst_share = max(worst_share, a)
            assert G["bgdist__" + k][0] <= INT_SHARE_CAP / 10, k  # measured over the whole stack, with room
            if cases.BACKGROUND[case]["filter_domain"] == "spatial":
                assert a == 0, k  # SciPy's two truncating passes, restated exactly
    assert worst_share <= INT_SHARE_CAP  # (of the stored pattern: one value of 3072 is 3.3e-4)


def known(cls, test):
    rows = {}
    prefix = f"known__{cls}__{test}__"
    for k in G.files:
        if k.startswith(prefix):
            i, n = k[len(prefix):].split("__")
            v = G[k]
            rows.setdefault(int(i), {})[n] = None if v.dtype.kind == "U" and str(v) == "None" else v
    return [rows[i] for i in sorted(rows)]


def test_known_answers_of_the_reference():
    p = DUMMY[0, 0]
    rows = known("TestGetDynamicBackgroundPattern", "test_get_dynamic_background_pattern_spatial")
    assert len(rows) == 3
    for r in rows:
        std = None if r["std"] is None else float(r["std"])
        bg = R.get_dynamic_background(p, "spatial", std, float(r["truncate"]))
        assert bg.dtype == np.uint8 and np.allclose(bg, r["answer"])
    rows = known("TestGetDynamicBackgroundPattern", "test_get_dynamic_background_frequency")
    assert len(rows) == 3
    for r in rows:
        a = r["answer"]
        bg = R.get_dynamic_background(p.astype(a.dtype), "frequency", float(r["std"]))
        assert bg.dtype == a.dtype and np.allclose(bg, a, atol=1e-4)
    # the chunk tests hand float32 patterns to the filter and store uint8: float32 background, then astype
    for r in known("TestGetDynamicBackgroundChunk", "test_get_dynamic_background_spatial"):
        bg = R.get_dynamic_background(p.astype(np.float32), "spatial", float(r["std"]))
        assert np.allclose(bg.astype(np.uint8), r["answer"])
    for r in known("TestGetDynamicBackgroundChunk", "test_get_dynamic_background_dtype_out"):
        a = r["answer"]
        bg = R.get_dynamic_background(p, "frequency", 2.0, dtype_out=a.dtype)
        assert bg.dtype == a.dtype and np.allclose(bg, a, atol=1e-4)


PLAN_PROBE = r"""
#include <cstdio>
#include "downsample_plan.h"
using namespace kpdi;
int main() {
  const int shapes[][3] = {{60, 60, 2}, {60, 60, 3}, {60, 60, 6}, {120, 120, 2}, {240, 240, 4}, {480, 480, 4}, {480, 480, 8},
                           {480, 480, 2}, {120, 96, 3}, {1024, 1024, 2}, {2048, 2048, 2}, {64, 48, 16}, {3, 3, 3}};
  for (int d = 0; d < 9; ++d)
    for (auto &s : shapes)
      for (int force = 0; force < 2; ++force) {
        const DsPlan p = ds_plan(d, s[0], s[1], s[2], 1000, force != 0);
        std::printf("%d %d %d %d %d %d %d %d %zu %zu %d %zu\n", d, s[0], s[1], s[2], force, p.path, p.threads, p.staged,
                    p.raw_bytes, p.lds_bytes, p.grid, p.workspace_bytes);
      }
  const DsPlan bad[] = {ds_plan(0, 60, 60, 1, 10), ds_plan(0, 60, 60, 7, 10), ds_plan(0, 60, 61, 2, 10), ds_plan(0, 60, 60, 2, 0),
                        ds_plan(6, 60, 60, 2, 10), ds_plan(0, 0, 60, 2, 10)};
  for (auto &p : bad) std::printf("bad %d\n", p.path);
  return 0;
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
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert lines[-6:] == ["bad -1"] * 6
    es = {0: 1, 1: 2, 2: 4, 3: 8, 4: 1, 5: 2}
    lds_cap, ws_cap = 60 * 1024, 256 << 20
    plans = {}
    for line in lines[:-6]:
        d, sy, sx, f, force, path, threads, staged, raw, lds, grid, ws = map(int, line.split())
        if d not in es:  # float16 / int32 / uint32 have no path
            assert path == -1
            continue
        nout = (sy // f) * (sx // f)
        binned = 4 * nout
        assert threads == (64 if nout <= 1024 else 256)
        if binned <= lds_cap and not force:
            raw16 = (sy * sx * es[d] + 15) // 16 * 16
            assert path == 0 and grid == 1000 and ws == 0
            assert staged == (raw16 + binned <= lds_cap) and raw == (raw16 if staged else 0) and lds == raw + binned
            assert lds <= lds_cap
        else:
            assert path == 1 and lds == 0 and staged == 0
            assert grid == max(1, min(1000, 1024, ws_cap // binned)) and ws == grid * binned <= ws_cap
        plans[(d, sy, sx, f, force)] = (path, staged, threads)
    assert plans[(0, 60, 60, 2, 0)] == (0, 1, 64)      # the 60 x 60 uint8 set: a wave per pattern, staged
    assert plans[(0, 240, 240, 4, 0)] == (0, 0, 256)   # 57.6 KB raw + 14.4 KB binned: binned from memory
    assert plans[(0, 480, 480, 4, 0)] == (0, 0, 256)   # 57.6 KB binned: the largest that stays in LDS
    assert plans[(0, 480, 480, 2, 0)][0] == 1 and plans[(3, 2048, 2048, 2, 0)][0] == 1
    assert plans[(3, 60, 60, 2, 0)] == (0, 1, 64) and plans[(0, 60, 60, 2, 1)][0] == 1


def test_error_messages_come_before_any_gpu_work():
    data = np.zeros((2, 60, 48), dtype=np.uint8)
    s = kpa.EBSD(data, static_background=np.ones((60, 48), dtype=np.uint8))
    det = s.detector
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        s.downsample(2, lazy_output=True)
    for bad in (2.5, 1, 0, -2, True, np.int64(2), "2"):
        with pytest.raises(ValueError) as e:
            s.downsample(bad)
        assert str(e.value) == f"Binning factor {bad} must be an integer > 1"
    with pytest.raises(ValueError) as e:
        s.downsample(5, inplace=False)
    assert str(e.value) == ("Binning factor 5 must be a divisor of the initial pattern shape (48, 60), but (3, 0) pixels "
                            "remain.\nYou might try to crop away these pixels first using EBSD.crop().")
    with pytest.raises(ValueError, match="dtype_out float16 is not supported"):
        s.downsample(2, dtype_out=np.float16)
    with pytest.raises(ValueError) as e:
        s.get_dynamic_background(filter_domain="emon")
    assert str(e.value) == "emon must be either of ['frequency', 'spatial']"
    with pytest.raises(TypeError, match=r"\['mode', 'sigma'\]"):
        s.get_dynamic_background("spatial", sigma=2, mode="nearest")
    with pytest.raises(ValueError, match="emon must be either of"):
        kpa.pattern.get_dynamic_background(data[0], filter_domain="emon")
    with pytest.raises(ValueError, match="Binning factor 7 must be a divisor"):
        kpa.pattern.downsample_stack(data, 7)
    # refused calls leave the signal as it was
    assert s.data is data and s.detector is det and det.shape == (60, 48) and det.binning == 1
    assert s.static_background.shape == (60, 48) and s._ctx is None


def test_signatures_lead_with_the_reference_parameters():
    def params(f):
        return [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()][1:]

    pk, ko, vk = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.VAR_KEYWORD
    e = inspect.Parameter.empty
    assert params(kpa.EBSD.downsample) == [("factor", e, pk), ("dtype_out", None, pk), ("show_progressbar", None, pk),
                                           ("inplace", True, pk), ("lazy_output", None, pk), ("devices", None, ko)]
    assert params(kpa.EBSD.get_dynamic_background) == [
        ("filter_domain", "frequency", pk), ("std", None, pk), ("truncate", 4.0, pk), ("dtype_out", None, pk),
        ("show_progressbar", None, pk), ("lazy_output", None, pk), ("devices", None, ko), ("kwargs", e, vk)]
    sig = inspect.signature(kpa.pattern.get_dynamic_background)
    assert list(sig.parameters)[:4] == ["pattern", "filter_domain", "std", "truncate"]
    assert [sig.parameters[n].default for n in ("filter_domain", "std", "truncate")] == ["frequency", None, 4.0]
    sig.bind(np.zeros((3, 3)), "spatial", 1, 4)
    inspect.signature(kpa.pattern.downsample_stack).bind(np.zeros((1, 4, 4)), 2, "uint8")
    inspect.signature(kpa.pattern.get_dynamic_background_stack).bind(np.zeros((1, 4, 4)), "frequency", None, 4.0, None)
    for name in ("downsample_stack", "get_dynamic_background", "get_dynamic_background_stack"):
        assert callable(getattr(kpa.pattern, name))
    assert _pattern.check_binning_factor(3, (60, 60)) == 3
