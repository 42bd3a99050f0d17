"""The builders of tests/_topk_cases.py against the float64 oracle, on the CPU: a wrong builder must not make a wrong
kernel look right in tests/test_gpu_topk_adversarial.py.  At the sizes the GPU test uses, on a sample of rows:

 * the constructed expectation IS the oracle's answer (ladders: index for index; plateaus: the index sets of every run of
   equal scores and the exact expected list, the oracle's own tie rule being lower index first too);
 * the top keep_n + 1 oracle scores of every sampled row are more than 2 x tie apart (tie = 2e-5, the default of
   `assert_topk_parity`), so that the parity check compares EVERY index - for float32 and for uint8 experimental
   patterns, for ncc and for ndp;
 * the orders are permutations, their inverses round-trip, and they are as hostile as they claim.
"""
import numpy as np
import pytest

import _topk_cases as tc
from oracle import c_oracle

KEEP_MAX = 70
SIZES = tc.SIZES   # (m, n, grains) of the GPU test


def sample_rows(m, count=64, seed=11):
    return np.arange(m) if m <= 300 else np.sort(np.random.default_rng(seed).choice(m, count, replace=False))


def oracle(case, exp, rows, keep_n):
    return c_oracle.rows_topk_f64(exp, case.dic, rows, case.metric, keep_n)


@pytest.mark.parametrize("metric", ["ncc", "ndp"])
@pytest.mark.parametrize("m,n,grains", SIZES)
def test_ladder_expectation_and_separation(m, n, grains, metric):
    base = tc.ladder(n, m, KEEP_MAX, grains, metric=metric)
    perm, inv = tc.order(base, "shuffled")
    case = base.reorder(perm)
    rows = sample_rows(m)
    for exp in (case.exp, case.exp_u8):
        s, i = oracle(case, exp, rows, KEEP_MAX + 1)
        assert tc.min_gap(s) > 2 * tc.TIE, tc.min_gap(s)
        assert np.array_equal(i, case.expected(KEEP_MAX + 1, rows))
        assert np.array_equal(perm[i], base.expected(KEEP_MAX + 1, rows))
        # distinct as float32 too: no exact tie between distinct entries (what bit-for-bit equivariance relies on)
        assert np.all(np.diff(s.astype(np.float32), axis=1) < 0)
    # the scores are the rungs: to float32 rounding for float32 patterns, to well under half a rung for uint8 images
    assert np.abs(s - case.expected_scores(KEEP_MAX + 1, rows)).max() < tc.SPACING / 2
    assert np.abs(oracle(case, case.exp, rows, 5)[0] - case.expected_scores(5, rows)).max() < 1e-6
    # 2 * keep_n well-separated rungs per grain, then the dense part
    g0 = np.sort(base.key[0][base.key[0] > 0])[::-1]
    assert np.all(-np.diff(g0[:2 * KEEP_MAX + 1]) > 2 * tc.TIE) and -np.diff(g0[2 * KEEP_MAX:]).max() < tc.SPACING / 2


def test_wider_rungs_for_reduced_precision():
    case = tc.ladder(12500, 300, 32, spacing=4 * 7e-4)
    s, i = oracle(case, case.exp, np.arange(0, 300, 7), 33)
    assert tc.min_gap(s) > 4 * 7e-4 - 1e-5 and np.array_equal(i, case.expected(33, np.arange(0, 300, 7)))
    with pytest.raises(AssertionError):
        tc.ladder(12500, 300, 70, spacing=0.01)  # 140 rungs of 0.01 do not fit: say so, do not squeeze them


@pytest.mark.parametrize("keep_n", [20, 70])
@pytest.mark.parametrize("m,n,grains", SIZES)
def test_orders_are_permutations_and_hostile(m, n, grains, keep_n):
    base = tc.ladder(n, m, keep_n, grains)
    rows = sample_rows(m, 16)
    want = base.expected(keep_n, rows)
    for name in tc.ORDERS:
        if name == "lane_concentrated" and n // tc.TILE < grains + 1:
            continue
        perm, inv = tc.order(base, name, keep_n)
        assert np.array_equal(np.sort(perm), np.arange(n))
        assert np.array_equal(inv[perm], np.arange(n)) and np.array_equal(perm[inv], np.arange(n))
        case = base.reorder(perm)
        got = case.expected(keep_n, rows)
        assert np.array_equal(perm[got], want) and np.array_equal(inv[want], got)
        for g in range(grains):
            mine = np.flatnonzero(case.key[g] > 0)          # this grain's entries, in dictionary order
            sc = case.key[g][mine]
            if name == "ascending":
                assert np.all(np.diff(sc) > 0)             # every entry beats all before it: 100 % of the rows see it
            elif name == "descending":
                assert np.all(np.diff(sc) < 0)
            elif name == "block_ascending":
                tile = mine // tc.TILE
                for t in range(1, tile.max() + 1):
                    assert sc[tile == t].min() > sc[tile == t - 1].max()
                assert all(np.all(np.diff(sc[tile == t]) < 0) for t in range(tile.max() + 1))
            elif name == "lane_concentrated":
                top = case.ranking(keep_n + 8)[g]
                assert len(np.unique(top // tc.TILE)) == 1     # one tile
                assert np.all((top % 32) % 8 // 4 == g % 2)    # the rows 4 h + {0..3} + 8 j of its 32-row groups
            elif name == "last_rows":
                top = case.ranking(keep_n + 8)[g]
                assert top.min() >= n - grains * (keep_n + 8)
                assert case.ranking(1)[g][0] >= n - 32 and n % tc.TILE != 0 and n % 32 != 0
    s, i = oracle(base.reorder(tc.order(base, "ascending")[0]), base.exp, rows, keep_n + 1)
    assert np.array_equal(tc.order(base, "ascending")[0][i], base.expected(keep_n + 1, rows))


def assert_plateau(case, rows, keep_n, start=0):
    """Oracle == expectation; neighbouring oracle scores are bit-equal (a plateau) or well separated."""
    s, i = oracle(case, case.exp, rows, keep_n + 1)
    want = case.expected(keep_n + 1, rows)
    assert np.array_equal(i, want)           # (the C oracle ranks ties by lower index, like the engine)
    d = -np.diff(s.astype(np.float64), axis=1)
    assert np.all((d == 0) | (d > 2 * tc.TIE)), d[(d != 0) & (d <= 2 * tc.TIE)]
    for r in range(len(rows)):               # the index SET of every run of equal scores
        for v in np.unique(s[r, :-1]):
            grp = s[r] == v
            if not grp[-1]:
                assert set(i[r, grp]) == set(want[r, grp])
    return s, i


@pytest.mark.parametrize("m,n,grains", SIZES)
def test_plateaus(m, n, grains):
    rows = sample_rows(m, 24)
    # 1: all identical
    case = tc.all_identical(n, m)
    s, i = oracle(case, case.exp, rows, 71)
    assert np.array_equal(i, np.tile(np.arange(71), (len(rows), 1))) and np.all(s == s[:, :1])
    assert np.array_equal(case.expected(70, rows, start=5000), np.tile(5000 + np.arange(70), (len(rows), 1)))
    for first in (256, 4096, 3 * 4096):   # ... with its lowest indices behind a ladder of lower scores
        if first + 71 <= n:
            case = tc.late_plateau(n, m, first)
            s, i = oracle(case, case.exp, rows, 71)
            assert np.array_equal(i, np.tile(first + np.arange(71), (len(rows), 1))) and np.all(s == s[:, :1])
            assert np.array_equal(i, case.expected(71, rows)) and case.key[0, :first].max() < case.key[0, first] - 2 * tc.TIE
    # 2: more copies of the best rung than any candidate buffer holds, contiguous and scattered
    for placement in ("contiguous", "scattered"):
        case = tc.plateau(n, m, 0, 320, placement, grains=grains)
        s, i = assert_plateau(case, rows, 70)
        assert np.all(s[:, 0] == s[:, 70])
        copies = [np.flatnonzero(k == k.max()) for k in case.key]
        assert all(len(c) == 321 for c in copies)
        if placement == "contiguous":    # (one run, but for the rung they copy and the well-separated rungs it steps over)
            assert np.sum(np.abs(copies[0] - np.median(copies[0])) < 400) >= 320
        else:                            # every tile holds some
            assert len(np.unique(copies[0] // tc.TILE)) >= min(n // tc.TILE, 200)
    # 3: r rungs, then a run of equal scores across the k-th place and across the pass boundaries (32; 20 on the wide form)
    for r, keep_ns in ((12, (20, 32, 33, 40, 70)), (25, (32, 33, 40, 70)), (1, (2,)), (0, (1,))):
        case = tc.plateau(n, m, r, 320, "scattered", grains=grains)
        s, i = assert_plateau(case, rows, 70)
        assert np.all(-np.diff(s[:, :r + 1], axis=1) > 2 * tc.TIE) and np.all(s[:, r] == s[:, 70])
        for keep_n in keep_ns:
            assert r < keep_n < r + 320
            want = case.expected(keep_n, rows)
            assert np.array_equal(want, i[:, :keep_n]) and np.all(np.diff(want[:, r:], axis=1) > 0)
    # 4: every rung negative, 300 degenerate patterns score exactly +0.0
    case = tc.zero_plateau(n, m, 300)
    s, i = assert_plateau(case, rows, 70)
    assert np.all(s == 0) and not np.signbit(s).any()
    flat = np.flatnonzero(case.dic.reshape(n, -1).min(axis=1) == case.dic.reshape(n, -1).max(axis=1))
    assert len(flat) == 300 and np.array_equal(i[0], flat[:71]) and len(np.unique(flat // tc.TILE)) >= min(n // tc.TILE, 200) - 1
    assert oracle(case, case.exp, rows[:4], 301)[0][:, 300].max() < -0.01
