"""The unbounded float32 match kernel (csrc/match32.hip: one step for whole tiles, one for the partial units of the last
round, the bound refresh between a tile's steps and its drain) at the shapes where that structure can go wrong - BIT FOR
BIT against match.hip (KPDI_F32_WIDE=0), and against the float64 oracle to the parity of every other sweep test (1e-5).

What a case reaches is asserted on the launch plan (`kpdi_plan_describe`, host arithmetic) and on the engine's counters,
so a change of the planner cannot quietly turn a case into another one:
  ring and peeling    steps per tile (kept pixels, padded to 24, / 24) = 1, 2, 3, 4, 7: the three-stage LDS ring wraps at
                      every phase, and with one step per tile the loads of a step belong to the tile after the next;
  tiles per workgroup 1, 2, 3, 4 whole tiles: the bound is refreshed behind the tiles 0, 1, 2 and 4 of a workgroup, and from
                      three rounds on the whole rounds are walked in a permuted order;
  tail mix            whole rounds only / + half units / + quarter units / a last tile with fewer than 256 valid rows.  A
                      launch of partial units ONLY does not exist: the planner never hands out fewer tiles than splits
                      (test_a_launch_always_starts_with_a_whole_round pins that), so the first unit of a workgroup is whole;
  set size, list      256, 512 and 4096 experimental patterns; keep_n 1 and 20; a signal mask whose padded pixel count
                      exceeds the kept pixels;
  bound               the rising ladder of tests/_topk_cases.py (every tile beats all tiles before it) on two tiles per
                      workgroup: a bound that is read late may only let more candidates through - the constructed answer
                      must come out on every row.
"""
import numpy as np
import pytest

import _topk_cases as tc
from oracle import kpdi_oracle as ko

SWITCHES = ("KPDI_F32_WIDE", "KPDI_TAIL_GEMM", "KPDI_TILE_ORDER", "KPDI_NO_TAIL")
WIDE = {"KPDI_F32_WIDE": "1", "KPDI_TAIL_GEMM": "0"}   # partial units inside the kernel, not tailgemm.hip
CLASSIC = {"KPDI_F32_WIDE": "0"}


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def sweep(monkeypatch, env, exp, dic, metric, keep_n, signal_mask=None):
    from kikuchipy_amd import _lib

    set_env(monkeypatch, env)
    code = {"ncc": _lib.METRIC_NCC, "ndp": _lib.METRIC_NDP}[metric]
    with _lib.Context(0) as c:
        c.set_problem(exp.shape[1], exp.shape[2], signal_mask, code, keep_n)
        c.set_experimental(exp)
        c.push_dictionary_chunk(dic, 0)
        s, i = c.finalize(keep_n)
        return s, i, c.counters()


def wide_plan(monkeypatch, m, n, k_kept, keep_n):
    from kikuchipy_amd import _lib

    set_env(monkeypatch, WIDE)
    return _lib.plan_describe(m, n, k_kept, keep_n, 256, 3)


#        m     n      sy  sx  masked metric keep  steps whole rounds, tail shift, rows of the last tile
CASES = [
    (4096, 4096,   4,  6, False, "ncc", 20, 1, 1, 0, 256),   # one step per tile, one tile per workgroup
    (4096, 8192,   6,  8, False, "ndp", 20, 3, 2, 0, 256),   # ndp: one more operand column (48 + 1 pixels: three steps)
    (4096, 12288,  8,  9, False, "ncc", 20, 3, 3, 0, 256),   # three rounds: the permuted order starts
    (4096, 16384,  8, 12, False, "ncc", 1, 4, 4, 0, 256),    # refreshes behind the tiles 0, 1, 2; keep_n = 1
    (4096, 20480,  4,  6, False, "ncc", 20, 1, 5, 0, 256),   # ... and behind tile 4, one step per tile
    (4096, 18332, 12, 14, False, "ncc", 20, 7, 4, 1, 156),   # 4 whole rounds + half units, a short last tile
    (4096, 4408,   6,  8, False, "ncc", 20, 2, 1, 2, 56),    # 1 whole round + quarter units, a short last tile
    (4096, 10240,  8,  9, False, "ncc", 1, 3, 2, 1, 256),    # 2 whole rounds + half units
    (256, 1500,    8,  9, False, "ncc", 1, 3, 1, 0, 220),    # one row block, a short last WHOLE tile
    (512, 4700,   10, 10, True, "ncc", 20, 4, 1, 0, 92),     # mask: 87 pixels kept, padded to 96
]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,sy,sx,masked,metric,keep_n,steps,rounds,shift,last_rows", CASES)
def test_match32_equals_match_hip_bit_for_bit(monkeypatch, m, n, sy, sx, masked, metric, keep_n, steps, rounds, shift,
                                              last_rows):
    rng = np.random.default_rng(m + n + sy)
    exp = rng.integers(0, 256, (m, sy, sx)).astype(np.uint8)
    dic = rng.random((n, sy, sx)).astype(np.float32)
    mask = None
    if masked:
        mask = np.zeros((sy, sx), dtype=bool)
        mask[0] = True
        mask[1:4, 0] = True
    kept = sy * sx - (0 if mask is None else int(mask.sum()))
    p = wide_plan(monkeypatch, m, n, kept, keep_n)
    assert p.form == 3 and p.launches == 1 and p.tail_gemm_rows == 0
    assert (p.tail_first if p.tail_shift else p.n_tiles) == rounds * p.nsplit and p.tail_shift == shift
    assert n - (p.n_tiles - 1) * 256 == last_rows
    wide = sweep(monkeypatch, WIDE, exp, dic, metric, keep_n, mask)
    classic = sweep(monkeypatch, CLASSIC, exp, dic, metric, keep_n, mask)
    assert wide[2]["match_form"] == 3 and classic[2]["match_form"] == 0
    assert wide[2]["kpad"] == 24 * steps and wide[2]["kpad"] >= kept + (metric == "ndp")
    assert np.array_equal(wide[0], classic[0]) and np.array_equal(wide[1], classic[1])
    rows = np.arange(m) if m <= 512 else np.sort(rng.choice(m, 64, replace=False))
    rs, ri = ko.dictionary_indexing(exp[rows], dic, metric=metric, keep_n=keep_n, signal_mask=mask)
    ko.assert_topk_parity(wide[0][rows], wide[1][rows], rs, ri, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("tile_order", ["permuted", "natural"])
def test_a_late_bound_drops_no_candidate_of_a_rising_ladder(monkeypatch, tile_order):
    """Every tile of the dictionary beats all tiles before it; two tiles per workgroup (natural order: the second tile of
    every workgroup holds its row's whole answer, screened with the bound read behind the first)."""
    m, n, keep_n = 4096, 8192, 20
    base = tc.ladder(n, m, keep_n_max=keep_n)
    perm, _ = tc.order(base, "ascending", keep_n)
    case = base.reorder(perm)
    p = wide_plan(monkeypatch, m, n, 480, keep_n)
    assert p.form == 3 and p.n_tiles == 2 * p.nsplit and p.tail_shift == 0
    env = dict(WIDE, **({"KPDI_TILE_ORDER": "natural"} if tile_order == "natural" else {}))
    s, i, cnt = sweep(monkeypatch, env, case.exp_u8, case.dic, "ncc", keep_n)
    assert cnt["match_form"] == 3
    assert np.array_equal(i, case.expected(keep_n))
    cs, ci, _ = sweep(monkeypatch, CLASSIC, case.exp_u8, case.dic, "ncc", keep_n)
    assert np.array_equal(s, cs) and np.array_equal(i, ci)
    rows = np.arange(0, m, 64)
    rs, ri = ko.dictionary_indexing(case.exp_u8[rows], case.dic, metric="ncc", keep_n=keep_n)
    ko.assert_topk_parity(s[rows], i[rows], rs, ri, atol=1e-5)


def test_a_launch_always_starts_with_a_whole_round(monkeypatch):
    """Why no case above runs partial units only: whatever the shape, the planner hands out at least as many tiles as
    splits, so the partial units (from tail_first on) never come first (host arithmetic, no GPU)."""
    for m in (1, 256, 300, 4096, 16384, 40000):
        for n_tiles in list(range(1, 40)) + [255, 256, 257, 391]:
            for tail in (256, 1):
                p = wide_plan(monkeypatch, m, (n_tiles - 1) * 256 + tail, 48, 20)
                assert p.form == 3 and p.n_tiles == n_tiles and 1 <= p.nsplit <= n_tiles
                if p.tail_shift:
                    assert p.tail_first >= p.nsplit and p.tail_first % p.nsplit == 0
