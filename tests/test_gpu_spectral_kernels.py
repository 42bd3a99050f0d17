"""The DFT kernels of the FFT filter (csrc/fftfilter.hip) and image quality (csrc/iq.hip) bit for bit: every case of
tests/_spectral_cases.py through `_lib.Context` against the restatement of its kernel path in the kernels' own arithmetic
(tests/_spectral_restate.py), with no tolerance: same dtype, same shape, values equal as numbers (-0 equal to +0), NaN
exactly where the restatement has NaN.  Image quality is compared on its float32 values the same way.

Path 1 (workspace) at small shapes and a second workspace batch are reached with KPDI_FFT_FILTER_PATH=1, KPDI_IQ_PATH=1
and KPDI_PATTERN_BATCH, read at each call.  The filter works in place, so its input is the sentinel of its result: a
batch that writes nowhere leaves the input standing.  Image quality gets a result array filled with a sentinel.

Nothing here is bounded rather than exact.  `sqrtf` and the f32 / f64 divisions of both files are correctly rounded in
the default build: the gfx950 assembly of iq.hip has v_sqrt_f32 followed by the two-sided one-ulp correction with
v_fma_f32 residuals, that of fftfilter.hip the v_div_scale / v_rcp / v_fma / v_div_fmas / v_div_fixup sequence."""

import os

import numpy as np
import pytest

import _spectral_cases as S
import _spectral_restate as R
from kikuchipy_amd import _lib
from test_gpu_prep_matrix import push_device

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(12345.0)  # no image quality: Q <= 1


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def set_switches(monkeypatch, c):
    for k in S.SWITCHES:
        assert k not in os.environ, k
    for k, v in S.env(c).items():
        monkeypatch.setenv(k, v)


def run(ctx, c, stack, upload=None):
    """The GPU result of case `c` on `stack`; `upload(ctx)` replaces set_experimental."""
    ctx.set_problem(c.shape[0], c.shape[1], None, _lib.METRIC_NCC, 1)
    if upload is None:
        ctx.set_experimental(stack)
    else:
        upload(ctx)
    if c.op == "iq":
        w, imax = S.iq_arguments(c.name) if c.name in S.CASES else (None, 0.0)
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        out = np.full(len(stack), SENTINEL, np.float32)
        _lib.check(ctx._f.image_quality(ctx._h, int(c.normalize), _lib._ptr(w), float(imax), _lib._ptr(out)))
        return out
    ctx.fft_filter(*S.table(c.name))
    return ctx.get_experimental()


def at(v, idx):
    """A stage value at a (pattern, y, x) or (pattern,) index, per-pattern values by the pattern alone."""
    if isinstance(v, tuple):
        return tuple(at(e, idx) for e in v)
    v = np.asarray(v)
    if v.ndim == 1:
        return v[idx[0]]
    idx = tuple(min(i, s - 1) for i, s in zip(idx, v.shape))  # (the half spectrum is narrower than the pattern)
    return v[idx[: v.ndim]]


def assert_same_bits(name, got, want, stages):
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    if same.all():
        return
    where = np.argwhere(~same)
    first = tuple(int(v) for v in where[0])
    held = {k: at(v, first) for k, v in stages.items()}
    raise AssertionError(f"{name}: {len(where)} of {got.size} values differ, first at {where[:5].tolist()}: got "
                         f"{got[first]!r}, restatement {want[first]!r}; its stages there: {held}")


@pytest.mark.parametrize("name", S.NAMES)
def test_case_equals_the_restatement_of_its_path(name, ctx, monkeypatch):
    c = S.CASES[name]
    set_switches(monkeypatch, c)
    want, stages = S.expected(name)
    got = run(ctx, c, S.stack(name))
    if c.op == "iq":
        assert not (got == SENTINEL).any(), (name, got)
    assert_same_bits(name, got, want, stages)


@pytest.mark.parametrize("name", [n for n, c in S.CASES.items()
                                  if c.path == 0 and c.op != "iq" and c.dtype not in ("float32", "float64")
                                  and n.replace("-p0-", "-p1-") in S.CASES])
def test_integer_stacks_same_bits_on_both_paths(name, ctx, monkeypatch):
    """The sums of integer patterns are exact, so the two paths may not differ in a single bit."""
    c0, c1 = S.CASES[name], S.CASES[name.replace("-p0-", "-p1-")]
    set_switches(monkeypatch, c0)
    a = run(ctx, c0, S.stack(c0.name))
    for k, v in S.env(c1).items():
        monkeypatch.setenv(k, v)
    b = run(ctx, c1, S.stack(c1.name))
    assert_same_bits(name, b, a, S.expected(name)[1])


@pytest.mark.parametrize("op", ["frequency", "iq"])
def test_switches_reach_the_workspace_path(op, ctx, monkeypatch):
    """On the `cancel` cases every pattern's result depends on the order of the path's f64 sums: the run without a
    switch and the run with it differ on every pattern, and each equals the restatement of its own path."""
    c0, c1 = (S.CASES[S.find("cancel", op, (60, 60), path, "float32")] for path in (0, 1))
    set_switches(monkeypatch, c0)
    a = run(ctx, c0, S.stack(c0.name))
    for k, v in S.env(c1).items():
        monkeypatch.setenv(k, v)
    b = run(ctx, c1, S.stack(c1.name))
    assert_same_bits(c0.name, a, *S.expected(c0.name))
    assert_same_bits(c1.name, b, *S.expected(c1.name))
    assert (a != b).reshape(len(a), -1).any(axis=1).all(), (a, b)


@pytest.mark.parametrize("shape", S.MISALIGNED_SHAPES)
@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
@pytest.mark.parametrize("op", S.OPS)
def test_misaligned_device_pointer(op, dtype, shape, ctx, monkeypatch):
    """Patterns handed over through set_experimental_dev one element behind a 256-byte boundary give the bits of the
    aligned run, which are the restatement's.  (The context copies what it is handed into its own buffer, so the
    kernels themselves see an aligned first pattern either way; within a stack they meet misaligned patterns whenever
    npix is no multiple of 4, which the shapes (7, 9), (6, 7) and (5, 5) of the table cover on both paths.)"""
    tf = {"frequency": "complex", "spatial": "even4", "iq": None}[op]
    c = S.Case(f"misaligned-{op}", op, shape, dtype, 3, tf, 0, False, None, True, False, "hash", 1000)
    for k in S.SWITCHES:
        assert k not in os.environ, k
    stack = S.hash_stack(shape, dtype, c.n, c.seed)
    table = None
    if op != "iq":
        from kikuchipy_amd.pattern._pattern import fft_filter_table

        _, shift, build = S.ff_cases.CASES[tf]
        table = fft_filter_table(build(shape, S.ff_cases.OurFunctions()), op, shift, shape)
        monkeypatch.setattr(S, "table", lambda name: table)
    aligned = run(ctx, c, stack)

    def upload(cx):
        push_device(cx, stack, stack.dtype.itemsize, lambda p: cx.set_experimental_dev(p, stack.dtype, len(stack)))

    offset = run(ctx, c, stack, upload)
    stages = {}
    if op == "iq":
        want = R.image_quality(stack, True, 0, stages=stages)
    else:
        want = R.fft_filter(stack, table[1], op, 0, stages=stages)
    assert_same_bits(c.name + " aligned", aligned, want, stages)
    assert_same_bits(c.name + " offset", offset, aligned, stages)
