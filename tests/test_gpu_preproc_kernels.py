"""Every kernel form of csrc/preproc.hip against tests/_preproc_restate.py, bit for bit: no tolerance and no share of
differing pixels - the kernels' arithmetic is fully specified (header of preproc.hip, docstring of the restatement).

The case table is tests/_preproc_cases.py; tests/test_host_preproc.py pins the restatement to the reference and every case
to the kernel form it names (the launcher's rules, restated there).  Covered here: the fused kernel with 256 and 1024
threads, unrolled (NT = 30 / 60) and generic, both boundary modes, windows of 1 to 70 taps (longer than the detector,
'reflect' beyond two periods), the last shape that fits the fused kernel and the first that does not, the streaming
kernels - static_stream_kernel, dynamic_stream_kernel<T, 0> and <T, 60> - and the second trip of the persistent loop;
both operations, scale_bg, static / dynamic / both; all six pattern dtypes; a device pointer one element off a 256-byte
boundary; the unrolled forms against the generic loop of a child process; and the degenerate patterns (0 / 0, x / 0,
constant, NaN, inf), whose results the reference defines."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _preproc_cases as C
import _preproc_generic_worker as worker
import _preproc_restate as R
from kikuchipy_amd import _lib
from oracle import kpdi_oracle as ko
from test_gpu_prep_matrix import push_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def same_bits(got, want):
    """Equal bits, NaN equal to NaN (the payload of a NaN is not part of the contract)."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and got[~nan].tobytes() == want[~nan].tobytes()


def describe(got, want):
    bad = ~((got == want) | (np.isnan(got.astype(np.float64)) & np.isnan(want.astype(np.float64))))
    where = np.argwhere(bad)[:4].tolist()
    return f"{int(bad.sum())} of {bad.size} pixels differ, first at {where}: got {got[bad][:4]}, want {want[bad][:4]}"


@functools.lru_cache(maxsize=None)
def inputs(c):
    p, bg = C.inputs(c, min(c.n, C.PERSISTENT_BASE))
    p.setflags(write=False)
    bg.setflags(write=False)
    return p, bg


@functools.lru_cache(maxsize=None)
def restated(c):
    """The restatement of a case's (first three) patterns: computed once, shared and read-only."""
    p, bg = inputs(c)
    out = R.preprocess(p, bg, **C.restate_kwargs(c))
    out.setflags(write=False)
    return out


def run(ctx, c, p, bg):
    ctx.reset_counters()
    out = worker.run(ctx, c, p, bg)
    assert ctx.counters()["preproc_launches"] == 1  # one call of the launcher: every recorded step
    return out


@pytest.mark.parametrize("c", C.WINDOWS + [C.STATIC_STREAM] + C.VARIANTS + C.DTYPE_CASES, ids=lambda c: c.name)
def test_kernel_form_equals_restatement(ctx, c):
    assert C.form(c) == c.form and "KPDI_PRE_GENERIC" not in os.environ
    p, bg = inputs(c)
    got = run(ctx, c, p, bg)
    assert same_bits(got, restated(c)), f"{c.name} ({' + '.join(c.form)}): {describe(got, restated(c))}"


def test_persistent_loop_takes_a_second_pattern(ctx):
    """516 patterns on dynamic_stream_kernel<T, 60>'s grid of 512: workgroups 0 - 3 reuse their scratch for a second
    pattern.  Pattern j is pattern j % 3, so every output must be its base pattern's, and those the restatement's."""
    c = C.PERSISTENT
    assert C.stream_grid(c.n) == 512 < c.n
    base, bg = inputs(c)
    p = base[np.arange(c.n) % C.PERSISTENT_BASE]
    got = run(ctx, c, p, bg)
    assert same_bits(got[:C.PERSISTENT_BASE], restated(c)), describe(got[:C.PERSISTENT_BASE], restated(c))
    wrong = [j for j in range(c.n) if not np.array_equal(got[j], got[j % C.PERSISTENT_BASE])]
    assert not wrong, f"patterns {wrong[:8]} ... differ from their base pattern (second trip: 512 - 515)"


@pytest.mark.parametrize("c", C.ALIGNMENT, ids=lambda c: c.name)
def test_offset_device_pointer(ctx, c):
    """Patterns handed over from device memory one element behind a 256-byte boundary: the same bits as the aligned run."""
    p, bg = inputs(c)
    aligned = run(ctx, c, p, bg)
    assert same_bits(aligned, restated(c)), describe(aligned, restated(c))
    ctx.set_problem(c.shape[0], c.shape[1], None, _lib.METRIC_NCC, 1)
    push_device(ctx, p, p.dtype.itemsize, lambda d: ctx.set_experimental_dev(d, p.dtype, len(p)))
    worker.record(ctx, c, bg, {"subtract": _lib.OP_SUBTRACT, "divide": _lib.OP_DIVIDE}[c.op])
    got = ctx.get_experimental()
    assert same_bits(got, aligned), describe(got, aligned)


def test_unrolled_equals_generic(ctx, tmp_path):
    """NT = 30 and NT = 60, fused and streaming, against the generic loop: one child process with KPDI_PRE_GENERIC=1 runs
    the five cases, this process runs them unrolled."""
    assert "KPDI_PRE_GENERIC" not in os.environ
    path = str(tmp_path / "generic.npy")
    child = subprocess.run([sys.executable, worker.__file__, path], env=dict(os.environ, KPDI_PRE_GENERIC="1"),
                           capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    generic = np.load(path)
    at = 0
    for c in C.GENERIC:
        assert C.form(c, generic=True) != C.form(c)
        p, bg = inputs(c)
        unrolled = run(ctx, c, p, bg)
        theirs = generic[at:at + unrolled.size].reshape(unrolled.shape)
        at += unrolled.size
        assert same_bits(unrolled, theirs), f"{c.name}: {describe(unrolled, theirs)}"
        assert same_bits(theirs, restated(c)), f"{c.name} (generic loop): {describe(theirs, restated(c))}"
    assert at == generic.size


@pytest.mark.parametrize("where", ["fused", "stream"])
@pytest.mark.parametrize("d", C.DEGENERATES, ids=lambda d: d.name)
def test_degenerate_patterns(ctx, d, where):
    """What the reference gives (tests/test_host_preproc.py holds the restatement to it): a NaN anywhere before a min or
    max makes the whole pattern NaN - 0 in the integer dtypes -, a constant pattern is 0 / 0, an infinite range sends the
    finite pixels to the bottom of the range.  The healthy patterns on either side are untouched by it."""
    c = C.degenerate_case(d, where)
    p, bg = C.degenerate_inputs(d, where)
    want = R.preprocess(p, bg, **C.restate_kwargs(c))
    got = run(ctx, c, p, bg)
    assert same_bits(got, want), f"{c.name} ({' + '.join(c.form)}): {describe(got, want)}"


def test_degenerate_row_is_prepared_as_zeros(ctx):
    """The fused preparation behind a degenerate pattern: an all-zero row, every score exactly 0 (the project's rule for
    degenerate rows, tests/test_gpu_degenerate.py), and the rows around it as the oracle has them."""
    rng = np.random.default_rng(21)
    exp = rng.integers(0, 256, (5, 60, 60), dtype=np.uint8)
    bg = rng.integers(1, 256, (60, 60), dtype=np.uint8)
    exp[2] = bg  # minus the background: constant, 0 / 0
    dic = rng.random((40, 60, 60), dtype=np.float32)
    mask = ~ko.circular_window((60, 60)).astype(bool)
    ctx.set_problem(60, 60, mask, _lib.METRIC_NCC, 10)
    ctx.set_experimental(exp)
    ctx.remove_static_background(bg.astype(np.float32), _lib.OP_SUBTRACT, False)
    ctx.remove_dynamic_background(_lib.OP_SUBTRACT, _lib.DOMAIN_FREQUENCY, 0.0, 4.0)
    ctx.reset_counters()
    ctx.push_dictionary_chunk(dic, 0)
    s, i = ctx.finalize(10)
    assert ctx.counters()["preproc_launches"] == 1
    u = ctx.get_experimental()
    assert same_bits(u, R.preprocess(exp, bg)) and not u[2].any()
    assert np.array_equal(s[2], np.zeros(10)) and not np.signbit(s[2]).any()
    live = [0, 1, 3, 4]
    rs, ri = ko.dictionary_indexing(u[live], dic, metric="ncc", keep_n=10, signal_mask=mask)
    ko.assert_topk_parity(s[live], i[live], rs, ri, atol=1e-5)
