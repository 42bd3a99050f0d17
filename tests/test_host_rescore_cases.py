"""The rescoring case table of tests/_rescore_cases.py without a GPU: the plain float64 model of rescore_kernel agrees with
the np.longdouble reference on every case within the float64 path's 1e-12; every named wrong variant of that model fails
tests/test_gpu_rescore.py's own check on some case (so the GPU test would notice a kernel wrong in that way); and the
table reaches every (experimental dtype x dictionary dtype) cell, every reduction length with and without a pix_map,
every window edge, every wave and workgroup position of the planted max_diff entry."""
import numpy as np
import pytest

import _rescore_cases as R


@pytest.fixture(scope="module")
def built():
    return {c.name: R.build(c.name) for c in R.CASES}


def test_the_model_agrees_with_the_precise_reference(built):
    worst = dict.fromkeys(R.GROUPS, 0.0)
    complaints = []
    for name, b in built.items():
        bad, w = R.check(b, *R.model(b))
        worst[b.case.group] = max(worst[b.case.group], w)
        complaints += [(name, line) for line in bad]
    print({g: f"{w:.2e}" for g, w in worst.items()})
    assert not complaints, complaints[:5]
    assert max(worst.values()) <= R.TOL / 10  # the reference side leaves the tolerance to the kernel


def test_the_reference_without_an_80_bit_long_double(built, monkeypatch):
    """Hosts whose np.longdouble is a double: exactly rounded sums (math.fsum) give the same expected scores."""
    if not R.LONG:
        pytest.skip("this host has no extended long double to compare with")
    monkeypatch.setattr(R, "LONG", False)
    for name in ("dtypes-int32-uint32-ncc", "dtypes-float16-float64-ndp", "length-257-mapped", "length-65-mapped", "length-3600"):
        b = built[name]
        kept = np.arange(b.k) if b.pix_map is None else b.pix_map
        for mi in range(b.case.m):
            got = R.precise_scores(b.exp[mi, kept], b.dic[:, kept], b.case.metric)
            cols = slice(b.case.cand_offset, b.case.cand_offset + b.case.n_cand)
            want = b.want[mi, cols]
            assert np.abs(got[b.cand_i[mi, cols] - b.case.global_start] - want).max() <= 2e-15, (name, mi)


def caught_by(fault, built):
    return [name for name, b in built.items() if R.check(b, *R.model(b, fault))[0]]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_a_wrong_kernel_fails_some_case(fault, built):
    caught = caught_by(fault, built)
    assert caught, fault
    # the three misread dtypes: in EVERY cell the dtype takes part in, both sides, both metrics
    misread = {"I8 read as U8": "int8", "U32 read as I32": "uint32", "F16 read as 2-byte integers": "float16"}
    if fault in misread:
        cells = [c.name for c in R.CASES if c.group == "dtypes" and misread[fault] in c.name.split("-")[1:3]]
        assert len(cells) == 34 and set(cells) <= set(caught), sorted(set(cells) - set(caught))
    positions = {"max_diff from wave 0 only": [f"maxdiff-{wg}-wave{w}" for wg in ("first", "middle", "last") for w in (1, 2, 3)],
                 "max_diff from the last workgroup only": [f"maxdiff-{wg}-wave{w}" for wg in ("first", "middle") for w in range(4)],
                 "max_diff overwritten instead of maxed": ["maxdiff-init-above"],
                 "max_diff including the -inf entries": ["maxdiff-skipped-entry"],
                 "pix_map[0] not used for the shift": ["length-65-mapped"],
                 "row_map ignored": ["rows-reversed", "rows-3-of-17"],
                 "degeneracy decided on the doubles": [c.name for c in R.CASES if c.group == "verdicts"]}
    assert set(positions.get(fault, ())) <= set(caught), sorted(set(positions[fault]) - set(caught))


def test_dtype_cells_and_data_ranges(built):
    cells = {(R.dtype_of(c.exp), R.dtype_of(c.dic), c.metric) for c in R.CASES if c.group == "dtypes"}
    assert cells == {(np.dtype(e), np.dtype(d), mt) for e in R.DTYPES for d in R.DTYPES for mt in (R.NCC, R.NDP)}
    assert len(cells) == 162
    for c in R.CASES:
        if c.group != "dtypes":
            continue
        assert (c.m, c.n_chunk, c.npix, c.k) == (5, 9, 132, 132)
        b = built[c.name]
        for a in (b.exp, b.dic):
            if a.dtype.kind == "i":  # a signedness slip must move the score
                assert (a < 0).mean() > 0.3 and a.min() < np.iinfo(a.dtype).min // 2 and a.max() > np.iinfo(a.dtype).max // 2
            if a.dtype == np.uint32:
                assert (a >= 2**31).mean() > 0.3
            if a.dtype.kind == "u":
                assert a.max() > np.iinfo(a.dtype).max // 2 + np.iinfo(a.dtype).max // 4
            if a.dtype == np.float16:
                mag = np.abs(a.astype(np.float64))
                assert ((mag > 0) & (mag < 2.0**-14)).sum() >= 5 and (mag > 60000).sum() >= 5 and np.isfinite(a).all()
                assert (a < 0).any()


def test_reduction_lengths_maps_and_rows(built):
    lengths = [c for c in R.CASES if c.group == "lengths"]
    assert sorted(c.k for c in lengths if c.pix is None) == sorted(R.LENGTHS)
    assert sorted({c.k for c in lengths if c.pix}) == sorted(R.LENGTHS)
    assert all(c.metric == R.NDP for c in lengths if c.k == 1)  # one pixel is a constant pattern under ncc
    assert {c.metric for c in lengths if c.k > 1} == {R.NCC, R.NDP}
    for c in R.CASES:
        b = built[c.name]
        big = c.k == 3600
        assert c.m <= 40 and c.n_chunk <= 64 and (c.npix <= 400 or big), c.name
        if b.pix_map is not None:  # a permutation of a strict subset, never monotone
            assert len(set(b.pix_map.tolist())) == c.k < c.npix and b.pix_map.min() >= 0 and b.pix_map.max() < c.npix
            assert c.k == 1 or (np.diff(b.pix_map) < 0).any(), c.name
    assert sum(c.k == 3600 for c in R.CASES) == 2  # the 60 x 60 pattern, whole and as a map into 61 x 61
    b = built["length-65-mapped"]  # the shift pixel is the brightest: 1e6 among values in [0, 1)
    first = b.pix_map[0]
    assert (b.exp[:, first] == 1e6).all() and (b.dic[:, first] == 1e6).all()
    rest = b.pix_map[1:]
    assert b.exp[:, rest].max() < 1 and b.dic[:, rest].max() < 1 and b.exp[:, rest].min() >= 0
    assert built["rows-reversed"].row_map.tolist() == [5, 4, 3, 2, 1, 0]
    b = built["rows-3-of-17"]
    assert b.row_map.tolist() == [16, 4, 9] and b.exp.shape[0] == 17 and b.case.m == 3


def test_window_edges(built):
    window = [c for c in R.CASES if c.group == "window"]
    assert {(c.global_start, c.cand_offset, c.n_cand) for c in window} == {(g, o, n) for g in (0, 1000) for o in (0, 5) for n in R.N_CANDS}
    for c in R.CASES:
        b = built[c.name]
        assert b.cand_s.shape[1] > c.cand_offset + c.n_cand  # something behind the window, always
        assert (b.kind[:, : c.cand_offset] == R.OUTSIDE).all() and (b.kind[:, c.cand_offset + c.n_cand:] == R.OUTSIDE).all()
        assert (b.kind[:, c.cand_offset: c.cand_offset + c.n_cand] != R.OUTSIDE).all()
        # what lies outside would be scored if read: a valid index
        outside = b.cand_i[b.kind == R.OUTSIDE]
        assert ((outside >= c.global_start) & (outside < c.global_start + c.n_chunk)).all()
    for c in window:
        b = built[c.name]
        lists = b.cand_i[:, c.cand_offset: c.cand_offset + c.n_cand]
        gs, n = c.global_start, c.n_chunk
        for edge, scored in ((gs - 1, False), (gs, True), (gs + n - 1, True), (gs + n, False), (R.INT_MAX, False)):
            at = np.argwhere(lists == edge)
            assert len(at), (c.name, edge)
            kinds = b.kind[:, c.cand_offset: c.cand_offset + c.n_cand][lists == edge]
            assert ((kinds >= R.DEGENERATE) if scored else (kinds == R.SKIPPED)).all(), (c.name, edge)
        if c.n_cand >= 3:
            assert lists[0, 1] == R.INT_MAX
        if c.n_cand >= 2:
            assert any(len(set(row.tolist())) < len(row) for row in lists), c.name  # duplicates within a list


def test_max_diff_cases(built):
    md = {c.name: built[c.name] for c in R.CASES if c.group == "maxdiff"}
    where = {(b.planted[0], (b.planted[1] - b.case.cand_offset) % 4) for name, b in md.items() if "wave" in name}
    assert where == {(mi, w) for mi in (0, 2, 4) for w in range(4)} and all(b.case.m == 5 for b in md.values())
    for name, b in built.items():  # every case: one planted entry, everything else a hundred times smaller
        sc = b.kind >= R.DEGENERATE
        if not sc.any():
            assert b.planted is None and b.want_md == b.init
            continue
        d = np.abs(b.want - b.cand_s.astype(np.float64))
        assert 2.9e-4 < d[b.planted] < 3.1e-4 and sc[b.planted], name
        d[b.planted] = 0
        assert d[sc].max() < 1.2e-6, name
    top = lambda b: np.float32(np.abs(b.want[b.planted] - np.float64(b.cand_s[b.planted])))
    assert md["maxdiff-init-zero"].init == 0 and md["maxdiff-first-wave0"].init == np.float32(1e-5)
    b = md["maxdiff-init-equal"]
    assert b.init == top(b) == b.want_md
    b = md["maxdiff-init-above"]
    assert b.init == b.want_md == np.float32(1e-2) > top(b)
    b = md["maxdiff-skipped-entry"]  # an offset a thousand times the planted one, on an entry that is not scored
    sk = b.kind == R.SKIPPED
    assert sk.any() and (b.cand_s[sk] == np.float32(0.5)).any() and b.want_md == top(b)
    assert (b.cand_i[sk] == R.INT_MAX).any() and (b.cand_i[sk] != R.INT_MAX).any()


def test_degenerate_rows_are_what_the_table_says(built):
    seen = set()
    for c in R.CASES:
        if c.deg_exp is None:
            continue
        b = built[c.name]
        for side, a, told in (("exp", b.exp, c.deg_exp), ("dic", b.dic, c.deg_dic)):
            got = tuple(R.degenerate32(a[r, b.pix_map], c.metric) for r in range(len(a)))
            assert got == told, (c.name, side, got, told)
        # and the expected output follows: 0 where either side is degenerate, a real score elsewhere
        deg = np.array(c.deg_exp)[:, None] | np.array(c.deg_dic)[None, :]
        assert np.array_equal(b.kind[:, : c.n_cand] == R.DEGENERATE, deg) and (b.kind[:, : c.n_cand][~deg] == R.ORDINARY).all()
        assert (b.want[:, : c.n_cand][deg] == 0).all() and (np.abs(b.want[:, : c.n_cand][~deg]) > 1e-6).all()
        seen.add((c.group, c.metric, R.dtype_of(c.exp).name))
        # a pixel that is not finite outside the kept area really is there
        if c.name.startswith("degenerate-f32"):
            kept = np.zeros(c.npix, bool)
            kept[b.pix_map] = True
            bad = ~np.isfinite(b.exp)
            assert (bad[:, kept].sum(axis=1) > 0).tolist() == [False, False, False, True, True, True, False, False, False, False]
            assert (bad[:, ~kept].sum(axis=1) > 0).tolist() == [False, False, False, False, False, False, True, True, True, True]
    assert seen == {(g, mt, d) for mt in (R.NCC, R.NDP) for g, d in (("degenerate", "uint8"), ("degenerate", "float32"),
                                                                    ("degenerate", "uint16"), ("verdicts", "float64"),
                                                                    ("verdicts", "float32"))}
    # uint16 at 60 000 with one pixel off by one is ordinary and far from it: its scores are real ones
    b = built["degenerate-u16-ncc"]
    assert (b.kind[1, [0, 1, 3]] == R.ORDINARY).all() and np.abs(b.want[1, 3]) > 1e-3
    # the three inputs on which the doubles and the float32 cast disagree: ordinary patterns in double
    b = built["degenerate-verdict-f64-ncc"]
    x = b.exp[:, b.pix_map]
    assert (x[1:].std(axis=1) > 0).all() and np.isfinite((x * x).sum(axis=1)).all()
    assert x[1].astype(np.float32).std() == 0
    with np.errstate(over="ignore"):
        c32 = x.astype(np.float32) - x.astype(np.float32).mean(axis=1, dtype=np.float64).astype(np.float32)[:, None]
        assert np.isinf((c32[2] * c32[2]).sum()) and (c32[3] * c32[3]).sum() == 0
