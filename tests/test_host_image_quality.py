"""Image quality (Krieger Lassen's Q) without a GPU: the frequency vectors, a float64 NumPy restatement of the
reference's arithmetic pinned to the reference's own known answers and to tests/golden/image_quality.npz (made by the
reference, tools/gen_image_quality_golden.py), how the three new callables bind, and the kernel path choice of
csrc/iq_plan.h compiled with the host compiler."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import _iq_inputs
import kikuchipy_amd as kpa
from conftest import GOLDEN, ROOT
from kikuchipy_amd.pattern import fft_frequency_vectors

IQ = np.load(os.path.join(GOLDEN, "image_quality.npz"))


def iq_f64(patterns, normalize=True, frequency_vectors=None, inertia_max=None):
    """Steps 1-6 of pattern/_pattern.py:698-775 in float64 (after the cast to float32); one value per pattern."""
    p = np.asarray(patterns).astype(np.float32).astype(np.float64)
    sy, sx = p.shape[-2:]
    fv = fft_frequency_vectors((sy, sx)) if frequency_vectors is None else np.asarray(frequency_vectors, np.float64)
    imax = fv.sum() / (sy * sx) if inertia_max is None else inertia_max
    if normalize:
        mean = p.mean(axis=(-2, -1), keepdims=True)
        std = p.std(axis=(-2, -1), keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = (p - mean) / std
    s = np.abs(np.fft.fft2(p))
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1 - ((s * fv).sum(axis=(-2, -1)) / s.sum(axis=(-2, -1))) / imax


def dummy():
    return np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"]


# tests/test_signals/test_ebsd.py:1893-1931 of the reference
DUMMY_NORM = np.array([[-0.0241, -0.0625, -0.0052], [-0.0317, -0.0458, -0.0956], [-0.1253, 0.0120, -0.2385]])
DUMMY_RAW = np.array([[0.2694, 0.2926, 0.2299], [0.2673, 0.1283, 0.2032], [0.1105, 0.2671, 0.2159]])


@pytest.mark.parametrize("shape, answer", [
    ((3, 3), [[1, 4, 1], [4, 7, 4], [1, 4, 1]]),
    ((5, 4), [[1, 4, 4, 1], [4, 7, 7, 4], [9, 12, 12, 9], [4, 7, 7, 4], [1, 4, 4, 1]]),
])
def test_fft_frequency_vectors(shape, answer):
    v = fft_frequency_vectors(shape)
    assert v.dtype == np.float64 and np.array_equal(v, np.array(answer, np.float64))


def test_fft_frequency_vectors_are_not_point_symmetric():
    v = fft_frequency_vectors((60, 60))
    assert v[0, 1] == 4 and v[0, 59] == 1


def test_restatement_known_answers():
    """tests/test_pattern/test_pattern.py:337-395 and tests/test_signals/test_ebsd.py:1893-1931 of the reference."""
    d = dummy()
    assert np.allclose(iq_f64(d, True), DUMMY_NORM, atol=1e-4)
    assert np.allclose(iq_f64(d, False), DUMMY_RAW, atol=1e-4)
    assert abs(iq_f64(d[0, 0], True) - -0.0241) < 1e-4 and abs(iq_f64(d[0, 0], False) - 0.2694) < 1e-4
    assert abs(iq_f64(d[2, 2], True) - -0.2385) < 1e-4
    rng = np.random.default_rng(0)
    assert abs(iq_f64(rng.random((1001, 1001)))) < 1e-2
    assert abs(iq_f64(np.full((1001, 1001), 5.0), normalize=False) - 1) < 1e-2


def fixture_cases():
    pre = np.load(os.path.join(GOLDEN, "preproc.npz"))
    for norm in (1, 0):
        yield f"ni__norm{norm}", pre["ni"], norm, {}
        yield f"ni_corrected__norm{norm}", pre["ni__static_then_dynamic"], norm, {}
        yield f"dummy__norm{norm}", dummy(), norm, {}
        fv, imax = IQ["custom__fv"], float(IQ["custom__inertia_max"])
        yield f"custom_fv__norm{norm}", pre["ni"], norm, {"frequency_vectors": fv}
        yield f"custom_imax__norm{norm}", pre["ni"], norm, {"inertia_max": imax}
        yield f"custom_both__norm{norm}", pre["ni"], norm, {"frequency_vectors": fv, "inertia_max": imax}
        for shape in _iq_inputs.SHAPES:
            for dtype in _iq_inputs.DTYPES:
                key = f"rand__{shape[0]}x{shape[1]}__{dtype}"
                yield f"{key}__norm{norm}", _iq_inputs.stack(shape, dtype, int(IQ[key + "__seed"])), norm, {}


def test_restatement_matches_fixture():
    """The reference computes in float32 (scipy.fft on complex64); the restatement in float64."""
    worst = 0.0
    for key, stack, norm, kw in fixture_cases():
        got = iq_f64(stack, bool(norm), **kw)
        want = IQ[key]
        assert got.shape == want.shape, key
        d = float(np.max(np.abs(got - want)))
        assert d < 1e-6, (key, d)
        worst = max(worst, d)
    print("largest |restatement - reference|:", worst)


# the three new callables, as the reference declares them (pattern/_pattern.py:698-703, :365,
# signals/ebsd.py:1312-1316); what this package adds is keyword-only with a default
SIGNATURES = {
    "pattern.get_image_quality": (["patterns", "normalize", "frequency_vectors", "inertia_max"],
                                  {"normalize": True, "frequency_vectors": None, "inertia_max": None}),
    "pattern.fft_frequency_vectors": (["shape"], {}),
    "EBSD.get_image_quality": (["self", "normalize", "show_progressbar"], {"normalize": True, "show_progressbar": None}),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures(name):
    import functools

    positional, defaults = SIGNATURES[name]
    f = functools.reduce(getattr, name.split("."), kpa)
    params = list(inspect.signature(f).parameters.values())
    assert [p.name for p in params if p.kind == p.POSITIONAL_OR_KEYWORD] == positional
    by_name = {p.name: p for p in params}
    for arg, default in defaults.items():
        assert by_name[arg].default is default or by_name[arg].default == default, (name, arg)
    for p in params:
        if p.name not in positional:
            assert p.kind == p.KEYWORD_ONLY and p.default is not p.empty, (name, p.name)


def test_input_validation_without_a_device():
    with pytest.raises(ValueError, match="frequency_vectors have shape"):
        kpa.pattern.get_image_quality(np.zeros((4, 5), np.uint8), frequency_vectors=np.ones((5, 4)))
    with pytest.raises(ValueError, match="inertia_max must be positive"):
        kpa.pattern.get_image_quality(np.zeros((4, 5), np.uint8), inertia_max=0)
    with pytest.raises(ValueError, match="two detector axes"):
        kpa.pattern.get_image_quality(np.zeros(5, np.uint8))


PLAN_PROBE = r"""
#include "iq_plan.h"
#include <cstdio>
int main() {
  long ns[] = {1L, 7L, 262144L};
  int sizes[] = {1, 2, 3, 8, 31, 59, 60, 61, 64, 96, 100, 128, 137, 138, 139, 140, 160, 200, 240, 480, 512, 1001, 1024, 2048};
  for (int sy : sizes)
    for (int sx : sizes)
      for (long n : ns) {
        kpdi::IqPlan p = kpdi::iq_plan(sy, sx, n);
        std::printf("%d %d %ld %d %zu %ld %d %zu %zu %zu", sy, sx, n, p.path, p.lds_bytes, (long)p.batch,
                    p.blocks_per_pattern, p.workspace_bytes, kpdi::iq_ws_pattern_bytes(sy, sx), kpdi::iq_lds_path_bytes(sy, sx));
        // the switches of the tests: unset (false, 0) is the plan above; forced to the workspace; forced and capped
        kpdi::IqPlan u = kpdi::iq_plan(sy, sx, n, false, 0), f = kpdi::iq_plan(sy, sx, n, true, 0),
                     c = kpdi::iq_plan(sy, sx, n, true, 3), k = kpdi::iq_plan(sy, sx, n, false, 3);
        const bool same = u.path == p.path && u.lds_bytes == p.lds_bytes && u.batch == p.batch &&
                          u.workspace_bytes == p.workspace_bytes && (p.path != 1 || u.blocks_per_pattern == p.blocks_per_pattern);
        std::printf(" %d %d %zu %ld %d %zu %d %ld %zu %d %ld %zu\n", (int)same, f.path, f.lds_bytes, (long)f.batch,
                    f.blocks_per_pattern, f.workspace_bytes, c.path, (long)c.batch, c.workspace_bytes, k.path, (long)k.batch,
                    k.workspace_bytes);
      }
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
    lds_cap, ws_cap, threads = 150 * 1024, 256 << 20, 256
    seen = set()
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if not line:
            continue
        sy, sx, n, path, lds, batch, bpp, ws, per, lds0 = map(int, line.split()[:10])
        same, fpath, flds, fbatch, fbpp, fws, cpath, cbatch, cws, kpath, kbatch, kws = map(int, line.split()[10:])
        inter = sy * (sx // 2 + 1)
        # what the LDS path holds: the intermediate (8 B per complex value), the f32 pattern, the twiddles
        assert lds0 >= inter * 8 + sy * sx * 4 + (sy + sx) * 8
        assert (path == 0) == (lds0 <= lds_cap), (sy, sx)
        seen.add(path)
        if path == 0:
            assert lds == lds0 <= lds_cap and batch == n and ws == 0
        else:
            assert path == 1, (sy, sx)  # every shape up to 2048 x 2048 has a path
            assert lds <= lds_cap
            assert 1 <= batch <= n and ws == batch * per <= ws_cap
            assert bpp * threads >= inter > (bpp - 1) * threads
            assert batch == n or (batch + 1) * per > ws_cap  # a batch is as large as the cap admits
        # KPDI_IQ_PATH / KPDI_PATTERN_BATCH unset change nothing; forced and capped plans meet the invariants of the
        # workspace path, and a cap alone leaves a shape of path 0 alone
        assert same == 1, (sy, sx, n)
        assert fpath == cpath == 1 and flds <= lds_cap, (sy, sx)
        assert 1 <= fbatch <= n and fws == fbatch * per <= ws_cap
        assert fbpp * threads >= inter > (fbpp - 1) * threads
        assert fbatch == n or (fbatch + 1) * per > ws_cap
        assert cbatch == min(fbatch, 3) and cws == cbatch * per
        if path == 1:
            assert (fbatch, fws, fbpp, flds) == (batch, ws, bpp, lds)
            assert (kpath, kbatch, kws) == (1, min(batch, 3), min(batch, 3) * per)
        else:
            assert (kpath, kbatch, kws) == (0, n, 0)
    assert seen == {0, 1}


def test_path_choice_known_shapes():
    """60 x 60 (the hot path) stays in LDS; 240 x 240 and 1024 x 1024 take the workspace."""
    from math import ceil

    def lds0(sy, sx):
        return sy * sx * 4 + sy * (sx // 2 + 1) * 8 + (sy + sx) * 8 + 128

    assert lds0(60, 60) < 150 * 1024 and lds0(240, 240) > 150 * 1024
    assert 1024 * 513 * 8 + 24 + ceil(1024 * 513 / 256) * 16 < 256 << 20
