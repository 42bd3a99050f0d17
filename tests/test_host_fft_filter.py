"""The FFT filter without a GPU: the three transfer-function builders against the reference's known answers, a float64
NumPy restatement of both domains pinned to tests/golden/fft_filter.npz (made by the reference,
tools/gen_fft_filter_golden.py), the Hermitian fold of the transfer function, argument errors, how the new callables
bind, and the kernel path choice of csrc/fftfilter_plan.h compiled with the host compiler."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.ndimage import correlate

import _fft_filter_cases as cases
import _iq_inputs
import kikuchipy_amd as kpa
from conftest import GOLDEN, ROOT
from kikuchipy_amd.filters import highpass_fft_filter, lowpass_fft_filter, modified_hann
from kikuchipy_amd.pattern import fft_filter_stack
from kikuchipy_amd.pattern._pattern import fft_filter_table

FF = np.load(os.path.join(GOLDEN, "fft_filter.npz"))
OURS = cases.OurFunctions()
RANGES = {np.uint8: (0, 255), np.uint16: (0, 65535), np.int8: (-128, 127), np.int16: (-32768, 32767),
          np.float32: (-1, 1), np.float64: (-1, 1)}


def _cast(v, dtype):
    """.astype with the package's definition of NaN: 0 for integer dtypes, NaN for float dtypes."""
    if np.issubdtype(dtype, np.integer):
        v = np.where(np.isnan(v), 0, v)
    return v.astype(dtype)


def _rescale(f, dtype):
    omin, omax = RANGES[np.dtype(dtype).type]
    if not np.all(np.isfinite(f)) or f.max() == f.min():
        return _cast(np.full(f.shape, np.nan), dtype)
    mn, mx = f.min(), f.max()
    return _cast(((f - mn) / (mx - mn)) * f.dtype.type(omax - omin) + f.dtype.type(omin), dtype)


def filter_f64(stack, domain, shift, tf):
    """EBSD.fft_filter restated: frequency `Re(ifft2(fft2(p) H'))` in complex128 and the rescale in float64; spatial
    the correlation with edge-replicated borders centred at (ty // 2, tx // 2) of the kernel rounded to float32, in
    float64, its float32 result rescaled in float32.  A non-finite pattern is NaN everywhere before the cast."""
    stack = np.asarray(stack)
    out = np.empty_like(stack)
    tf = np.asarray(tf)
    for idx in np.ndindex(stack.shape[:-2]):
        p = stack[idx].astype(np.float32).astype(np.float64)
        if not np.all(np.isfinite(p)):
            f = np.full(p.shape, np.nan)
        elif domain == "frequency":
            h = np.fft.ifftshift(tf) if shift else tf
            f = np.real(np.fft.ifft2(np.fft.fft2(p) * h))
        else:
            w = tf.astype(np.float32).astype(np.float64)
            f = correlate(p, w, mode="nearest").astype(np.float32)
        out[idx] = _rescale(f, stack.dtype)
    return out


def case_f64(stack, name):
    domain, shift, build = cases.CASES[name]
    return filter_f64(stack, domain, shift, build(stack.shape[-2:], OURS))


# Ties: the rescaled value of a pixel can be an integer in exact arithmetic, and then the reference's FFT round-off
# decides on which side of it the truncation falls.  Kernels with integer taps on integer patterns (sobel, circ7, k3x7)
# make such ties common: measured up to 0.63 % of the pixels (circ7 on uint16), against at most 0.18 % for the other
# cases (complex on uint16) and none for the frequency-domain cases on the Ni patterns.
INTEGER_KERNELS = {"sobel", "circ7", "k3x7"}


def assert_close(got, want, label, int_frac=2e-3, atol=1e-6):
    """Integer outputs: at most one grey level apart, on at most `int_frac` of the pixels; float outputs: `atol`."""
    assert got.dtype == want.dtype and got.shape == want.shape, label
    if np.issubdtype(got.dtype, np.integer):
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert d.max() <= 1, (label, d.max())
        assert np.count_nonzero(d) / d.size <= int_frac, (label, np.count_nonzero(d) / d.size)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=atol, err_msg=label)


def tie_fraction(name):
    return 1e-2 if name in INTEGER_KERNELS else 2e-3


# ---- the transfer functions (tests/test_filters/test_window.py:282-430 of the reference, restated) --------------------

@pytest.mark.parametrize("shape, c, w_c, answer", [
    ((5, 5), 1, 1, [[0.0012, 0.0470, 0.1353, 0.0470, 0.0012], [0.0470, 0.7095, 1.0, 0.7095, 0.0470],
                    [0.1353, 1.0, 1.0, 1.0, 0.1353], [0.0470, 0.7095, 1.0, 0.7095, 0.0470],
                    [0.0012, 0.0470, 0.1353, 0.0470, 0.0012]]),
    ((6, 5), 2, 1, [[0.0057, 0.0670, 0.1353, 0.0670, 0.0057], [0.2534, 0.8945, 1.0, 0.8945, 0.2534],
                    [0.8945, 1.0, 1.0, 1.0, 0.8945], [1.0, 1.0, 1.0, 1.0, 1.0], [0.8945, 1.0, 1.0, 1.0, 0.8945],
                    [0.2534, 0.8945, 1.0, 0.8945, 0.2534]]),
])
def test_lowpass_known_answers(shape, c, w_c, answer):
    w = lowpass_fft_filter(shape=shape, cutoff=c, cutoff_width=w_c)
    assert w.shape == shape and w.dtype == np.float64
    np.testing.assert_allclose(w, answer, atol=1e-4)


@pytest.mark.parametrize("shape, c, w_c, answer", [
    ((5, 5), 2, 2, [[1, 1, 1, 1, 1], [1, 0.8423, 0.6065, 0.8423, 1], [1, 0.6065, 0.1353, 0.6065, 1],
                    [1, 0.8423, 0.6065, 0.8423, 1], [1, 1, 1, 1, 1]]),
    ((6, 5), 2, 1, [[1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 0.5034, 0.1353, 0.5034, 1], [1, 0.1353, 0.0003, 0.1353, 1],
                    [1, 0.5034, 0.1353, 0.5034, 1], [1, 1, 1, 1, 1]]),
])
def test_highpass_known_answers(shape, c, w_c, answer):
    w = highpass_fft_filter(shape=shape, cutoff=c, cutoff_width=w_c)
    assert w.shape == shape and w.dtype == np.float64
    np.testing.assert_allclose(w, answer, atol=1e-4)


def test_cutoff_width_defaults_to_half_the_cutoff():
    np.testing.assert_array_equal(lowpass_fft_filter((96, 96), 30), lowpass_fft_filter((96, 96), 30, 15))
    np.testing.assert_array_equal(highpass_fft_filter((96, 96), 30), highpass_fft_filter((96, 96), 30, 15))


@pytest.mark.parametrize("nx, answer", [
    (3, [0.5, 1, 0.5]),
    (11, [0.1423, 0.4154, 0.6548, 0.8412, 0.9594, 1.0, 0.9594, 0.8412, 0.6548, 0.4154, 0.1423]),
])
def test_modified_hann_known_answers(nx, answer):
    np.testing.assert_allclose(modified_hann(Nx=nx), answer, atol=1e-4)


def test_window_still_refuses_the_named_fft_windows():
    with pytest.raises(NotImplementedError, match="custom window"):
        kpa.filters.Window("lowpass", (5, 5), cutoff=2)


# ---- the restatement against the reference's own results --------------------------------------------------------------

@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_matches_the_reference_on_ni(name):
    pre = np.load(os.path.join(GOLDEN, "preproc.npz"))
    assert_close(case_f64(pre["ni"], name), FF[f"ni__{name}"], name, tie_fraction(name))
    if name in cases.NI_CORRECTED_CASES:
        assert_close(case_f64(pre["ni__static_then_dynamic"], name), FF[f"ni_corrected__{name}"], name,
                     tie_fraction(name))


@pytest.mark.parametrize("dtype", _iq_inputs.DTYPES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_restatement_matches_the_reference_on_the_dummy(name, dtype):
    dummy = np.load(os.path.join(GOLDEN, "di_dummy.npz"))["dummy"].astype(dtype)
    # 81 pixels of values 0 - 255 at most: ties up to 7 of them (lowhigh); the reference's float32 result of a 6 x 5
    # kernel on 3 x 3 patterns (big) is 3e-6 off the float64 one
    assert_close(case_f64(dummy, name), FF[f"dummy__{dtype}__{name}"], (name, dtype), int_frac=8 / 81, atol=5e-6)


def synthetic_keys():
    return sorted(k for k in FF.files if k.startswith("rand__") and k.count("__") == 2)


@pytest.mark.parametrize("key", synthetic_keys())
def test_restatement_matches_the_reference_on_synthetic_stacks(key):
    _, shape, dtype = key.split("__")
    shape = tuple(int(v) for v in shape.split("x"))
    stack = _iq_inputs.stack(shape, dtype, int(FF[key + "__seed"]))[: cases.N_STORED]
    name = str(FF[key + "__case"])
    assert_close(case_f64(stack, name), FF[key], key, 5e-2 if shape == (1, 64) else tie_fraction(name))


def test_fixture_covers_every_case_and_stored_shape():
    stored = {str(FF[k + "__case"]) for k in synthetic_keys()}
    assert stored == set(cases.NAMES)
    assert {k.split("__")[1] for k in synthetic_keys()} == {f"{a}x{b}" for a, b in _iq_inputs.SHAPES if a * b <= 128 * 96}
    assert os.path.getsize(os.path.join(GOLDEN, "fft_filter.npz")) < 1 << 20


def test_degenerate_patterns_restated():
    z = np.zeros((2, 6, 7), np.uint8)
    z[1] = 9
    f = np.zeros((2, 6, 7), np.float32)
    f[0, 2, 3] = np.nan
    f[1, 0, 0] = np.inf
    h = lowpass_fft_filter((6, 7), 2)
    for dom, tf in (("frequency", h), ("spatial", np.ones((3, 3)))):
        np.testing.assert_array_equal(filter_f64(z, dom, True, tf), 0)
        assert np.isnan(filter_f64(f, dom, True, tf)).all()


# ---- the Hermitian fold ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(6, 8), (7, 9), (6, 9), (1, 16), (16, 1), (5, 5)])
@pytest.mark.parametrize("shift", [False, True])
def test_hermitian_fold_equals_the_full_complex_inverse(shape, shift):
    rng = np.random.default_rng(sum(shape) + shift)
    p = rng.random(shape).astype(np.float32).astype(np.float64)
    for h in (rng.standard_normal(shape) + 1j * rng.standard_normal(shape), np.arange(np.prod(shape)).reshape(shape)):
        want = np.real(np.fft.ifft2(np.fft.fft2(p) * (np.fft.ifftshift(h) if shift else h)))
        domain, table = fft_filter_table(h, "frequency", shift, shape)
        assert domain == kpa._lib.DOMAIN_FREQUENCY and table.shape == (shape[0], shape[1] // 2 + 1)
        got = np.fft.irfft2(np.fft.rfft2(p) * table, s=shape)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))


def test_shift_of_odd_shapes_is_the_references_fftshift_multiply_ifftshift():
    rng = np.random.default_rng(3)
    p, h = rng.random((5, 7)), rng.random((5, 7))
    ref = np.real(np.fft.ifft2(np.fft.ifftshift(np.fft.fftshift(np.fft.fft2(p)) * h)))
    np.testing.assert_allclose(np.real(np.fft.ifft2(np.fft.fft2(p) * np.fft.ifftshift(h))), ref, atol=1e-13)


# ---- arguments and signatures ------------------------------------------------------------------------------------------

def test_argument_errors_without_a_device():
    p = np.zeros((2, 4, 5), np.uint8)
    with pytest.raises(ValueError, match=r"^fourier must be either of \['frequency', 'spatial'\]$"):
        fft_filter_stack(p, np.ones((4, 5)), "fourier")
    with pytest.raises(ValueError, match="transfer_function has shape"):
        fft_filter_stack(p, np.ones((5, 4)), "frequency")
    with pytest.raises(ValueError, match="spatial kernel must be a real 2D array"):
        fft_filter_stack(p, np.ones(3), "spatial")
    with pytest.raises(ValueError, match="two detector axes"):
        fft_filter_stack(np.zeros(5, np.uint8), np.ones(5), "frequency")
    with pytest.raises(ValueError, match=r"'lazy_output=True' requires 'inplace=False'"):
        kpa.EBSD(p).fft_filter(np.ones((4, 5)), "frequency", lazy_output=True)


def _leading(f, n):
    return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[:n]]


def test_signatures_lead_with_the_references_parameters():
    e = inspect.Parameter.empty
    assert _leading(kpa.EBSD.fft_filter, 7) == [("self", e), ("transfer_function", e), ("function_domain", e),
                                                ("shift", False), ("show_progressbar", None), ("inplace", True),
                                                ("lazy_output", None)]
    extra = list(inspect.signature(kpa.EBSD.fft_filter).parameters.values())[7:]
    assert all(p.kind == p.KEYWORD_ONLY for p in extra)
    for f in (kpa.filters.lowpass_fft_filter, kpa.filters.highpass_fft_filter):
        assert _leading(f, 3) == [("shape", e), ("cutoff", e), ("cutoff_width", None)]
    assert _leading(kpa.filters.modified_hann, 1) == [("Nx", e)]


# ---- the path choice ---------------------------------------------------------------------------------------------------

PLAN_PROBE = r"""
#include "fftfilter_plan.h"
#include <cstdio>
int main() {
  long ns[] = {1L, 7L, 262144L};
  int sizes[] = {1, 2, 3, 8, 31, 59, 60, 61, 64, 96, 100, 110, 111, 112, 128, 137, 138, 139, 140, 160, 200, 240, 480,
                 512, 1001, 1024, 2048};
  for (int d = 0; d < 2; ++d)
    for (int sy : sizes)
      for (int sx : sizes)
        for (long n : ns) {
          kpdi::FfPlan p = kpdi::ff_plan(d, sy, sx, n);
          std::printf("%d %d %d %ld %d %zu %ld %d %d %zu %zu %zu", d, sy, sx, n, p.path, p.lds_bytes, (long)p.batch,
                      p.blocks_half, p.blocks_pix, p.workspace_bytes, kpdi::ff_ws_pattern_bytes(d, sy, sx),
                      kpdi::ff_lds_path_bytes(d, sy, sx));
          // the switches of the tests: unset (false, 0) is the plan above; forced to the workspace; forced and capped
          kpdi::FfPlan u = kpdi::ff_plan(d, sy, sx, n, false, 0), f = kpdi::ff_plan(d, sy, sx, n, true, 0),
                       c = kpdi::ff_plan(d, sy, sx, n, true, 3), k = kpdi::ff_plan(d, sy, sx, n, false, 3);
          const bool same = u.path == p.path && u.lds_bytes == p.lds_bytes && u.batch == p.batch &&
                            u.workspace_bytes == p.workspace_bytes &&
                            (p.path != 1 || (u.blocks_half == p.blocks_half && u.blocks_pix == p.blocks_pix));
          std::printf(" %d %d %zu %ld %d %d %zu %d %ld %zu %d %ld %zu\n", (int)same, f.path, f.lds_bytes, (long)f.batch,
                      f.blocks_half, f.blocks_pix, f.workspace_bytes, c.path, (long)c.batch, c.workspace_bytes, k.path,
                      (long)k.batch, k.workspace_bytes);
        }
  std::printf("bad %d\n", kpdi::ff_plan(2, 60, 60, 1).path);
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
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert lines[-2] == "bad -1"
    big = {}
    for line in lines[:-2]:
        d, sy, sx, n, path, lds, batch, bh, bp, ws, per, lds0 = map(int, line.split()[:12])
        same, fpath, flds, fbatch, fbh, fbp, fws, cpath, cbatch, cws, kpath, kbatch, kws = map(int, line.split()[12:])
        inter, npix4 = sy * (sx // 2 + 1), (sy * sx + 3) // 4 * 4
        if d == 0:  # the pattern, two complex intermediates, the twiddles
            assert lds0 >= npix4 * 4 + 2 * inter * 8 + (sy + sx) * 8
            assert per >= 2 * inter * 8 >= sy * sx * 4  # (the f32 result reuses the second intermediate)
        else:  # the pattern and the result
            assert lds0 >= 2 * npix4 * 4 and per >= npix4 * 4
        assert (path == 0) == (lds0 <= lds_cap), (d, sy, sx)
        seen.add((d, path))
        if path == 0:
            assert lds == lds0 <= lds_cap and batch == n and ws == 0
        else:
            assert path == 1, (d, sy, sx)  # every shape up to 2048 x 2048 has a path
            assert lds <= lds_cap
            assert 1 <= batch <= n and ws == batch * per <= ws_cap
            assert bh * threads >= inter > (bh - 1) * threads
            assert bp * threads >= sy * sx > (bp - 1) * threads
            assert batch == n or (batch + 1) * per > ws_cap  # a batch is as large as the cap admits
        # KPDI_FFT_FILTER_PATH / KPDI_PATTERN_BATCH unset change nothing; forced and capped plans meet the invariants of
        # the workspace path, and a cap alone leaves a shape of path 0 alone
        assert same == 1, (d, sy, sx, n)
        assert fpath == cpath == 1 and flds <= lds_cap, (d, sy, sx)
        assert 1 <= fbatch <= n and fws == fbatch * per <= ws_cap
        assert fbh * threads >= inter > (fbh - 1) * threads and fbp * threads >= sy * sx > (fbp - 1) * threads
        assert fbatch == n or (fbatch + 1) * per > ws_cap
        assert cbatch == min(fbatch, 3) and cws == cbatch * per
        if path == 1:
            assert (fbatch, fws, fbh, fbp, flds) == (batch, ws, bh, bp, lds)
            assert (kpath, kbatch, kws) == (1, min(batch, 3), min(batch, 3) * per)
        else:
            assert (kpath, kbatch, kws) == (0, n, 0)
        big[(d, sy, sx, n)] = (path, batch)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the hot shape stays in LDS in both domains; 240 x 240 and 1024 x 1024 take the workspace in the frequency domain
    assert big[(0, 60, 60, 262144)][0] == 0 and big[(1, 60, 60, 262144)][0] == 0
    assert big[(0, 240, 240, 7)][0] == 1 and big[(0, 1024, 1024, 7)] == (1, 7)
    assert big[(1, 1024, 1024, 262144)][0] == 1 and big[(0, 2048, 2048, 1)] == (1, 1)
