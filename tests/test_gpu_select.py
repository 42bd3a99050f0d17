"""kpdi_select_patterns and kpdi_set_navigation_mask on the GPU (csrc/select.hip through `_lib.Context`), bit for bit
against NumPy indexing: every pattern dtype, detectors below, at and above the 16-byte piece, rectangles that take each of
the three kernel paths with every source alignment, pattern counts inside one workgroup and across two, and index lists
in any order.  The refusals are argument checks that return before a launch."""

import numpy as np
import pytest

from _select_cases import COUNTS, DETECTORS, DTYPES, index_lists, probe, rectangles
from kikuchipy_amd import _lib

pytestmark = pytest.mark.gpu

def expected(p, idx, rows, cols):
    r = np.arange(rows[0], rows[0] + rows[1] * rows[2], rows[1])[: rows[2]]
    c = np.arange(cols[0], cols[0] + cols[1] * cols[2], cols[1])[: cols[2]]
    q = p if idx is None else p[idx]
    return np.ascontiguousarray(q[:, r][:, :, c])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def contexts():
    with _lib.Context(0) as src, _lib.Context(0) as dst:
        yield src, dst


def load(ctx, p):
    ctx.set_problem(p.shape[1], p.shape[2], None, _lib.METRIC_NCC, 1)
    ctx.set_experimental(p)


@pytest.mark.parametrize("detector", DETECTORS, ids=lambda d: f"{d[0]}x{d[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_selection_into_another_context(contexts, dtype, detector):
    """The whole table through the two-context form, which leaves the source resident for the next selection."""
    src, dst = contexts
    sy, sx = detector
    n_checked = 0
    for n in COUNTS:
        p = probe(n, sy, sx, dtype)
        load(src, p)
        for name, rows, cols in rectangles(sy, sx):
            for lname, idx in index_lists(n):
                src.select_patterns(idx, rows, cols, into=dst)
                got = dst.get_experimental()
                assert same(got, expected(p, idx, rows, cols)), (n, name, lname)
                n_checked += 1
        assert same(src.get_experimental(), p), n  # the source is unchanged
    assert n_checked >= len(COUNTS) * 9 * 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place_equals_into_another_context(contexts, dtype):
    src, dst = contexts
    for sy, sx in DETECTORS:
        p = probe(7, sy, sx, dtype)
        for name, rows, cols in rectangles(sy, sx):
            idx = np.array([6, 0, 3, 3, 5])
            load(src, p)
            src.select_patterns(idx, rows, cols, into=dst)
            src.select_patterns(idx, rows, cols)
            a, b = src.get_experimental(), dst.get_experimental()
            assert same(a, b) and same(a, expected(p, idx, rows, cols)), (sy, sx, name)
            assert src._detector == (rows[2], cols[2]) and src.n_experimental == 5


def test_in_place_identity_keeps_the_patterns(contexts):
    src, _ = contexts
    p = probe(7, 12, 10, "uint16")
    load(src, p)
    src.select_patterns()
    assert same(src.get_experimental(), p)


@pytest.mark.parametrize("into_other", [False, True])
@pytest.mark.parametrize("rect", ["full", "col0=1", "steps 2 and 3"])
def test_recorded_static_background_runs_before_the_selection(contexts, rect, into_other):
    """A recorded (not yet run) static background step is applied to the patterns the selection picks from; into
    another context the source keeps both its patterns and the recorded step."""
    src, dst = contexts
    rng = np.random.default_rng(3)
    p = rng.integers(0, 256, (7, 12, 10)).astype(np.uint8)
    bg = rng.integers(1, 256, (12, 10)).astype(np.float32)
    load(src, p)
    src.remove_static_background(bg)
    want_all = src.get_experimental()  # (runs the step)
    assert not same(want_all, p)
    rows, cols = {n: (r, c) for n, r, c in rectangles(12, 10)}[rect]
    idx = np.array([4, 1, 1, 6])
    load(src, p)
    src.remove_static_background(bg)
    src.select_patterns(idx, rows, cols, into=dst if into_other else None)
    got = (dst if into_other else src).get_experimental()
    assert same(got, expected(want_all, idx, rows, cols))
    if into_other:
        assert same(src.get_experimental(), want_all)  # its step is still recorded and runs now


@pytest.mark.parametrize("recorded", [False, True])
def test_a_destination_with_a_problem_of_the_new_shape_keeps_its_keep_n_and_metric(recorded):
    """dst has a problem of the selection's shape with its own keep_n and metric, src another keep_n: dst keeps its own -
    in the engine as in the Python context - also when src's recorded step sends the selection through a copy of the
    whole set in dst; one without such a problem takes src's."""
    rng = np.random.default_rng(8)
    p = rng.integers(0, 256, (9, 12, 10)).astype(np.uint8)
    bg = rng.integers(1, 256, (12, 10)).astype(np.float32)
    dic = rng.random((40, 12, 9)).astype(np.float32)
    with _lib.Context(0) as src, _lib.Context(0) as dst, _lib.Context(0) as fresh, _lib.Context(0) as plain:
        src.set_problem(12, 10, None, _lib.METRIC_NCC, 5)
        src.set_experimental(p)
        if recorded:
            src.remove_static_background(bg)
        dst.set_problem(12, 9, None, _lib.METRIC_NDP, 2)
        src.select_patterns(cols=(1, 1, 9), into=dst)
        src.select_patterns(cols=(1, 1, 9), into=fresh)
        want = src.get_experimental()[:, :, 1:]
        assert same(dst.get_experimental(), want) and same(fresh.get_experimental(), want)
        assert dst._keep_n == 2 and fresh._keep_n == 5

        def run(ctx):
            ctx.push_dictionary_chunk(dic, 0)
            return ctx.finalize()

        # the same patterns uploaded under each problem: what the engine must answer
        for ctx, metric, k in ((dst, _lib.METRIC_NDP, 2), (fresh, _lib.METRIC_NCC, 5)):
            s, i = run(ctx)
            plain.set_problem(12, 9, None, metric, k)
            plain.set_experimental(want)
            ws, wi = run(plain)
            assert s.shape == (9, k) and np.array_equal(s, ws) and np.array_equal(i, wi), k


def test_whole_copy_carries_recorded_steps(contexts):
    """The identity selection into another context (what deepcopy uses) with steps recorded: both contexts then hold
    the processed patterns."""
    src, dst = contexts
    rng = np.random.default_rng(4)
    p = rng.integers(0, 256, (7, 12, 10)).astype(np.uint8)
    load(src, p)
    src.remove_static_background(rng.integers(1, 256, (12, 10)).astype(np.float32))
    src.remove_dynamic_background()
    src.select_patterns(into=dst)
    a, b = dst.get_experimental(), src.get_experimental()
    assert same(a, b) and not same(a, p)


def test_refusals_leave_the_resident_set(contexts):
    src, dst = contexts
    p = probe(7, 12, 10, "float32")
    load(src, p)
    bad = [
        dict(pattern_index=np.array([], dtype=np.int64)),          # n_out < 1
        dict(pattern_index=[0, 7]),                                # index outside [0, m_all)
        dict(pattern_index=[-1]),
        dict(rows=(0, 0, 3)),                                      # step < 1
        dict(cols=(0, -1, 3)),
        dict(rows=(0, 1, 13)),                                     # rows leave the detector
        dict(rows=(2, 3, 5)),
        dict(rows=(-1, 1, 2)),
        dict(cols=(4, 1, 7)),                                      # columns leave the detector
        dict(cols=(0, 4, 4)),
        dict(rows=(0, 1, 0)),
    ]
    for kw in bad:
        for into in (None, dst):
            with pytest.raises(_lib.KpdiError, match="libkpdi error"):
                src.select_patterns(into=into, **kw)
            assert same(src.get_experimental(), p), kw
    # a signal mask while the shape changes; the same mask is fine while it does not
    mask = np.zeros((12, 10), dtype=bool)
    mask[0] = True
    src.set_problem(12, 10, mask, _lib.METRIC_NCC, 1)
    with pytest.raises(_lib.KpdiError, match="signal mask"):
        src.select_patterns(cols=(1, 1, 9))
    assert same(src.get_experimental(), p)
    src.select_patterns([2, 1])
    assert same(src.get_experimental(), p[[2, 1]])
    # no resident patterns
    with _lib.Context(0) as empty:
        with pytest.raises(_lib.KpdiError, match="kpdi_set_experimental"):
            empty.select_patterns(into=dst)
        with pytest.raises(_lib.KpdiError, match="kpdi_set_experimental"):
            empty.set_navigation_mask(None)


def test_held_chunks_refuse_a_new_shape(contexts):
    src, _ = contexts
    rng = np.random.default_rng(5)
    p = rng.random((7, 12, 10)).astype(np.float32)
    src.set_problem(12, 10, None, _lib.METRIC_NCC, 1)
    src.set_experimental(p)
    src.hold_dictionary_chunk(rng.random((9, 12, 10)).astype(np.float32), 0)
    try:
        with pytest.raises(_lib.KpdiError, match="held"):
            src.select_patterns(rows=(0, 1, 6))
        assert same(src.get_experimental(), p)
    finally:
        src.release_held()


@pytest.mark.skipif(_lib.device_count() < 2, reason="needs two GPUs")
def test_contexts_on_different_devices_are_refused(contexts):
    src, _ = contexts
    p = probe(7, 5, 7, "uint8")
    load(src, p)
    with _lib.Context(1) as other:
        with pytest.raises(_lib.KpdiError, match="devices"):
            src.select_patterns(into=other)
    assert same(src.get_experimental(), p)


def test_set_navigation_mask_matches_an_upload_with_the_mask():
    """Indexing after kpdi_set_navigation_mask equals indexing after an upload that brought the mask, and clearing it
    equals an upload without one."""
    rng = np.random.default_rng(6)
    exp = rng.random((20, 12, 10)).astype(np.float32)
    dic = rng.random((50, 12, 10)).astype(np.float32)
    nav = np.zeros(20, dtype=bool)
    nav[[0, 5, 6, 19]] = True

    def run(ctx):
        ctx.reset_topk()
        ctx.push_dictionary_chunk(dic, 0)
        return ctx.finalize()

    with _lib.Context(0) as a, _lib.Context(0) as b:
        for c in (a, b):
            c.set_problem(12, 10, None, _lib.METRIC_NCC, 3)
        a.set_experimental(exp, nav)
        b.set_experimental(exp)
        before = b.counters()["h2d_bytes"]
        b.set_navigation_mask(nav)
        (sa, ia), (sb, ib) = run(a), run(b)
        assert sa.shape == (16, 3) and np.array_equal(sa, sb) and np.array_equal(ia, ib)
        b.set_navigation_mask(None)
        a.set_experimental(exp)
        (sa, ia), (sb, ib) = run(a), run(b)
        assert sa.shape == (20, 3) and np.array_equal(sa, sb) and np.array_equal(ia, ib)
        # only the dictionary went up again, never the patterns
        assert b.counters()["h2d_bytes"] - before == 2 * dic.nbytes
        assert same(b.get_experimental(), exp)
