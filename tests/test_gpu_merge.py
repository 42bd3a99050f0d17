"""The top-k merge kernels on their own (kpdi_merge_selftest, kpdi_merge64_selftest, kpdi_fill_selftest): every case of
tests/_merge_cases.py through every kernel of csrc/merge.hip that can hold it, each forced by name, against the NumPy
reference - bit for bit on scores, exact on indices, the caller's sentinel outside the merged columns and the poison behind
every list's count included.  tests/test_host_merge_cases.py shows which forks the table reaches and that a merge that
ignored counts, broke ties by memory order, skipped the segments or dropped the last slot would fail here."""
import numpy as np
import pytest

import _merge_cases as M
from kikuchipy_amd import _lib

pytestmark = pytest.mark.gpu

HIP_INVALID_VALUE = 1


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def run(ctx, c, b, force):
    seg = None if b.segments is None else b.segments
    return ctx.merge_selftest(b.sources, c.m, c.k, b.out_s, b.out_i, out_offset=c.out_offset, segments=seg,
                              seg_sources=M.seg_mask(c), force=force)


@pytest.mark.parametrize("c", M.CASES, ids=M.case_id)
def test_every_kernel_returns_the_reference(ctx, c):
    b = M.build(c)
    want_s, want_i = M.reference(c, b)
    auto = M.plan_of(M.candidates(c))
    for force in [-1] + M.plans_for(c):
        got_s, got_i, err, ran = run(ctx, c, b, force)
        assert err == 0 and ran == (auto if force < 0 else force), (force, err, ran)
        bad = np.argwhere((got_s.view(np.uint32) != want_s.view(np.uint32)) | (got_i != want_i))
        assert not len(bad), (M.PLANS[ran], "forced" if force >= 0 else "auto", len(bad), bad[:4].tolist(),
                              [(got_s[r, q], got_i[r, q], want_s[r, q], want_i[r, q]) for r, q in bad[:4]])
    assert M.plans_for(c)[0] == auto


def test_a_kernel_too_small_is_refused_and_nothing_runs(ctx):
    c = M.BY_NAME["total-769"]
    b = M.build(c)
    for force in (0, 1, 7, 99, -2):
        got_s, got_i, err, ran = run(ctx, c, b, force)
        assert err == HIP_INVALID_VALUE and ran == -1
        assert (got_s == M.SENTINEL_S).all() and (got_i == M.SENTINEL_I).all()
    with pytest.raises(_lib.KpdiError, match="end at element"):  # an extent behind its buffer never reaches the GPU
        ctx.merge_selftest([dict(b.sources[0], row_stride=b.sources[0]["row_stride"] + 1)] + list(b.sources[1:]), c.m, c.k,
                           b.out_s, b.out_i)
    with pytest.raises(_lib.KpdiError, match="out_offset"):
        ctx.merge_selftest(b.sources, c.m, c.k, b.out_s, b.out_i, out_offset=1)


def run64(ctx, c):
    run_, cs, ci, row_stride, list_stride = M.build64(c)
    out_s = np.full((c.m, c.k), M.SENTINEL64_S)
    out_i = np.full((c.m, c.k), M.SENTINEL64_I, np.int32)
    return ctx.merge64_selftest(c.k, cs, ci, c.lists, c.len, row_stride, list_stride, out_s, out_i, run=run_,
                                in_place=c.in_place, cert=M.cert_inputs(c) if c.cert is not None else None)


@pytest.mark.parametrize("c", M.CASES64, ids=M.case_id)
def test_f64_merge(ctx, c):
    """`fewer-than-k`: the ranks behind the entries keep the caller's content and the pattern is not counted as
    uncertified (tests/_merge_cases.py: reference64)."""
    want_s, want_i, want_unc = M.reference64(c)
    got_s, got_i, unc, err = run64(ctx, c)
    assert err == 0
    assert np.array_equal(got_s.view(np.uint64), want_s.view(np.uint64)) and np.array_equal(got_i, want_i)
    assert unc == want_unc


def test_f64_merge_refuses_more_than_150_kb(ctx):
    got_s, got_i, unc, err = run64(ctx, M.LDS_REFUSED._replace(in_place=False))
    assert err == HIP_INVALID_VALUE
    assert (got_s == M.SENTINEL64_S).all() and (got_i == M.SENTINEL64_I).all()


@pytest.mark.parametrize("name", M.FILL_LAUNCHES)
def test_fill_segments(ctx, name):
    ranges = M.FILL_LAUNCHES[name]
    got = ctx.fill_selftest(M.fill_buffer(ranges), ranges)
    want = M.fill_reference(ranges)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (len(bad), bad[:8].tolist(), [hex(v) for v in got[bad[:8]]])
