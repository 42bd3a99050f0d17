"""The fused top-k of every match kernel form on inputs whose answer is known by construction (tests/_topk_cases.py; the
builders are checked against the oracle on the CPU by tests/test_host_topk_cases.py): ladders of well-separated scores in
hostile dictionary orders, and plateaus of bit-equal scores longer than any candidate buffer, laid across the k-th place
and across the pass boundaries of keep_n > 32.

Checks, strongest first: (1) the indices ARE the constructed answer, on every row; (2) `assert_topk_parity` against the
float64 oracle on every row (up to 300) or a fixed sample of 64; (3) every order gives the shuffled order's result bit for
bit once the indices are mapped back, and so do the f32 forms among themselves and profiling level 3 against none; (4) the
slow paths really ran: the epilogue counters of profiling level 3.

Which input reaches which path is listed in DESIGN.md ("Adversarial inputs of the fused top-k").

KPDI_TOPK_PROFILE=<file>: what the runs measured (kernel form, splits, bound plan, appended candidates per list, overflow
events, the float16 score error that set the float16 rung spacing, wall time) is written there as JSON -
profiles/topk_adversarial.json is such a file.
"""
import functools
import json
import os
import time

import numpy as np
import pytest

import _topk_cases as tc
from oracle import c_oracle
from oracle import kpdi_oracle as ko

pytestmark = pytest.mark.gpu

SWITCHES = ("KPDI_F32_WIDE", "KPDI_TAIL_GEMM", "KPDI_TILE_ORDER", "KPDI_NO_TAIL", "KPDI_F16_WAVES", "KPDI_UPLOAD_TILES")
F32, F16X2, F16, F64 = 0, 1, 2, 3   # _lib.COMPUTE_*
# name: (compute, switches, match_form counter, has candidate buffers)
FORMS = {
    "match.hip": (F32, {"KPDI_F32_WIDE": "0"}, 0, False),
    "match.hip no tail": (F32, {"KPDI_F32_WIDE": "0", "KPDI_NO_TAIL": "1"}, 0, False),
    "wide tail-kernel": (F32, {"KPDI_F32_WIDE": "1", "KPDI_TAIL_GEMM": "1"}, 3, True),
    "wide tail-kernel natural": (F32, {"KPDI_F32_WIDE": "1", "KPDI_TAIL_GEMM": "1", "KPDI_TILE_ORDER": "natural"}, 3, True),
    "wide units": (F32, {"KPDI_F32_WIDE": "1", "KPDI_TAIL_GEMM": "0"}, 3, True),
    "wide units natural": (F32, {"KPDI_F32_WIDE": "1", "KPDI_TAIL_GEMM": "0", "KPDI_TILE_ORDER": "natural"}, 3, True),
    "f16 8 waves": (F16, {"KPDI_F16_WAVES": "8"}, 2, True),
    "f16 8 waves natural": (F16, {"KPDI_F16_WAVES": "8", "KPDI_TILE_ORDER": "natural"}, 2, True),
    "f16 4 waves": (F16, {"KPDI_F16_WAVES": "4"}, 2, True),
    "f16 4 waves natural": (F16, {"KPDI_F16_WAVES": "4", "KPDI_TILE_ORDER": "natural"}, 2, True),
    "split-f16": (F16X2, {}, 1, False),
    "float64": (F64, {}, None, False),
}
F32_FORMS = [f for f, v in FORMS.items() if v[0] == F32]
KEEP_NS = (1, 2, 20, 32, 33, 40, 70)
SMALL, MID, LARGE = tc.SIZES
PLAIN = (16384, 1800, 2)   # 64 row blocks x 4 splits of 2 tiles each (plan.h: choose_nsplit): 16 lists per pattern < keep_n = 20 -
                           # bound_rank 2, the 8-entry candidate buffers

RECORDS = {"cases": [], "f16_score_error": None, "wall_s": {}}


def dump_records():
    path = os.environ.get("KPDI_TOPK_PROFILE")
    if path:
        with open(path, "w") as f:
            json.dump(RECORDS, f, indent=1)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    RECORDS["wall_s"][request.node.name] = round(time.time() - t0, 2)
    RECORDS["wall_s_total"] = round(sum(v for v in RECORDS["wall_s"].values()), 1)
    dump_records()


class Engine:
    """One context of one kernel form (the switches are read by `set_problem`)."""

    def __init__(self, monkeypatch, form, profiling=None, extra=None):
        from kikuchipy_amd import _lib

        self.form = form
        self.compute, env, self.match_form, self.buffers = FORMS[form]
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in {**env, **(extra or {})}.items():
            monkeypatch.setenv(k, v)
        self.ctx = _lib.Context(0)
        self.profiling = profiling
        if profiling:
            self.ctx.set_profiling(profiling)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def sweep(self, exp, dic, metric, keep_n, push="one", start=0):
        """(scores, indices, counters) of `dic` pushed at dictionary index `start` the way `push` says."""
        from kikuchipy_amd import _lib

        c = self.ctx
        n = len(dic)
        code = {"ncc": _lib.METRIC_NCC, "ndp": _lib.METRIC_NDP}[metric]

        def run(pieces):
            c.set_problem(exp.shape[1], exp.shape[2], None, code, keep_n, self.compute)
            c.set_experimental(exp)
            c.reset_counters()
            for a, b in pieces:
                c.push_dictionary_chunk(dic[a:b], start + a)
            return c.finalize(keep_n)

        if push == "shards":   # 8 'ranks', merged in the engine's merge order (test_sharded_sweep_equals_full_sweep)
            from kikuchipy_amd.parallel import shard_range

            parts = [run([shard_range(n, r, 8)]) for r in range(8)]
            s = np.concatenate([p[0] for p in parts], axis=1)
            i = np.concatenate([p[1] for p in parts], axis=1)
            o = np.lexsort((i, -s), axis=1)[:, :keep_n]
            return np.take_along_axis(s, o, 1), np.take_along_axis(i, o, 1), c.counters()
        cuts = {"one": [0, n], "three": [0, n // 5, n // 5 + n // 2 + 37, n], "small": list(range(0, n, 700)) + [n]}[push]
        s, i = run(list(zip(cuts[:-1], cuts[1:])))
        return s, i, c.counters()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def sample(m):
    return np.arange(m) if m <= 300 else np.sort(np.random.default_rng(11).choice(m, 64, replace=False))


@functools.lru_cache(maxsize=6)
def ladder(size, keep_max, metric="ncc", spacing=tc.SPACING):
    m, n, grains = size
    return tc.ladder(n, m, keep_max, grains, spacing, metric)


@functools.lru_cache(maxsize=8)
def ordered(size, keep_max, name, metric="ncc", spacing=tc.SPACING, keep_n=20):
    base = ladder(size, keep_max, metric, spacing)
    perm, inv = tc.order(base, name, keep_n)
    return base.reorder(perm), perm


@functools.lru_cache(maxsize=8)
def plateau_case(size, kind, r=0, spacing=tc.SPACING):
    m, n, grains = size
    if kind == "identical":
        return tc.all_identical(n, m)
    if kind == "zeros":
        return tc.zero_plateau(n, m, 300)
    if kind == "late":
        return tc.late_plateau(n, m, r)
    return tc.plateau(n, m, r, 320, kind, grains=grains, spacing=spacing)


def oracle_for(eng, case, exp, rows, keep_n, start=0):
    """The float64 oracle's best keep_n of the rows: float64 dot products of the prepared float32 rows (oracle/c_oracle.py);
    for the float64 arithmetic the oracle evaluated in float64 throughout, as tests/test_gpu_f64.py does."""
    if eng.compute == F64:
        s, i = ko.dictionary_indexing(exp[rows], case.dic, metric=case.metric, keep_n=keep_n, dtype=np.float64)
        return s, i + start
    return c_oracle.rows_topk_f64(exp, [(start, case.dic)], rows, case.metric, keep_n)


def atol_of(eng):
    # the project's tolerances: test_gpu_engine.py (f32, split-f16: 1e-5; f16: 2e-3), test_gpu_f64.py (1e-12)
    return {F32: 1e-5, F16X2: 1e-5, F16: 2e-3, F64: 1e-12}[eng.compute]


def record(eng, label, size, keep_n, cnt, **more):
    m = size[0]
    row_blocks = (m + 255) // 256
    grid = cnt["match_grid"]
    nsplit = grid // row_blocks if grid % row_blocks == 0 and grid >= row_blocks else cnt["match_nsplit"]
    lists = (4 if eng.buffers else 2) * nsplit
    list_len = 1 if keep_n <= 1 else 8 if keep_n <= 8 else 20 if keep_n <= 20 else 32   # match.hip: match_list_len
    rank = 1 if lists >= 32 else -(-list_len // lists)                                  # kernels.h: bound_plan
    plan = "grouped" if lists >= 32 else "plain, rank %d" % rank
    rec = {"case": label, "form": eng.form, "m": m, "n": size[1], "keep_n": keep_n, "match_form": cnt["match_form"],
           "nsplit": nsplit, "lists_per_pattern": lists, "bound_plan": plan}
    if eng.profiling == "epilogue" and eng.buffers:
        rec.update(appended_per_list=round(cnt["epi_appended"] / max(cnt["epi_lists"], 1), 3), overflows=cnt["epi_overflows"],
                   first_tiles_direct=cnt["epi_direct_first"])
    rec.update(more)
    RECORDS["cases"].append(rec)
    if eng.match_form is not None:
        assert cnt["match_form"] == eng.match_form, (eng.form, cnt["match_form"])
    return rec


def check(eng, case, exp, s, i, keep_n, start=0, exact=True):
    """(1) the constructed answer on every row, (2) oracle parity on the sample."""
    m = len(exp)
    if exact:
        want = case.expected(keep_n, start=start)
        bad = np.flatnonzero((i != want).any(axis=1))
        assert bad.size == 0, f"{eng.form}: {bad.size} rows differ from the constructed answer; row {bad[0]}: {i[bad[0]]} != {want[bad[0]]}"
    rows = sample(m)
    rs, ri = oracle_for(eng, case, exp, rows, keep_n, start)
    ko.assert_topk_parity(s[rows], i[rows], rs, ri, atol=atol_of(eng))


@pytest.fixture(scope="module")
def f16_spacing():
    """Rung spacing of the float16 ladders: 4 x the largest float16 score error |engine - float64 oracle| measured on the
    shuffled order of the same ladder (never below the spacing the uint8 images need)."""
    from kikuchipy_amd import _lib

    case, _ = ordered(MID, 70, "shuffled")
    rows = sample(MID[0])
    with _lib.Context(0) as c:
        c.set_problem(24, 20, None, _lib.METRIC_NCC, 70, _lib.COMPUTE_F16)
        c.set_experimental(case.exp_u8)
        c.push_dictionary_chunk(case.dic, 0)
        s, i = c.finalize(70)
    rs, ri = c_oracle.rows_topk_f64(case.exp_u8, case.dic, rows, "ncc", 70)
    err = float(np.abs(s[rows].astype(np.float64) - rs).max())
    spacing = max(tc.SPACING, 4 * err)
    RECORDS["f16_score_error"] = {"max_abs_error": err, "rows": len(rows), "keep_n": 70, "rung_spacing": spacing,
                                  "uint8_floor": tc.SPACING}
    print(f"float16 score error {err:.3e} -> rung spacing {spacing:.3e}")
    return spacing


def spacing_of(form, f16_spacing):
    return f16_spacing if FORMS[form][0] == F16 else tc.SPACING


@pytest.mark.parametrize("form", list(FORMS))
def test_every_order_gives_the_constructed_answer_bit_for_bit(monkeypatch, form, f16_spacing):
    """keep_n = 20, every order x this form: uint8 experimental patterns against 12 500 entries (grouped plan), float32
    patterns against 1 500 entries (one row block: fewer than 32 lists per pattern); ascending also against 28 300."""
    sp = spacing_of(form, f16_spacing)
    with Engine(monkeypatch, form) as eng:
        for size, u8, orders in ((MID, True, tc.ORDERS), (SMALL, False, tc.ORDERS), (LARGE, False, ("shuffled", "ascending"))):
            ref = None
            for name in orders:
                case, perm = ordered(size, 20, name, "ncc", sp)
                exp = case.exp_u8 if u8 else case.exp
                s, i, cnt = eng.sweep(exp, case.dic, "ncc", 20)
                record(eng, "ladder " + name, size, 20, cnt)
                check(eng, case, exp, s, i, 20)
                if name == "shuffled":
                    ref = (bits(s), perm[i])
                    # no exact ties between distinct entries in the top keep_n + 1 (oracle scores rounded to float32)
                    rs, _ = c_oracle.rows_topk_f64(exp, case.dic, sample(len(exp)), "ncc", 21)
                    assert np.all(np.diff(rs.astype(np.float32), axis=1) < 0)
                else:
                    assert np.array_equal(perm[i], ref[1]), name
                    assert np.array_equal(bits(s), ref[0]), f"{name}: scores differ from the shuffled order's as bit patterns"


@pytest.mark.parametrize("form", list(FORMS))
def test_ndp_orders(monkeypatch, form, f16_spacing):
    sp = spacing_of(form, f16_spacing)
    with Engine(monkeypatch, form) as eng:
        ref = None
        for name in ("shuffled", "ascending", "block_ascending"):
            case, perm = ordered(MID, 20, name, "ndp", sp)
            s, i, cnt = eng.sweep(case.exp_u8, case.dic, "ndp", 20)
            record(eng, "ndp ladder " + name, MID, 20, cnt)
            check(eng, case, case.exp_u8, s, i, 20)
            if ref is None:
                ref = (bits(s), perm[i])
            else:
                assert np.array_equal(perm[i], ref[1]) and np.array_equal(bits(s), ref[0]), name


@pytest.mark.parametrize("form", list(FORMS))
def test_every_keep_n_on_rising_scores_and_on_a_plateau_across_the_kth_place(monkeypatch, form, f16_spacing):
    """keep_n = 1 ... 70 (21 ... 32 on the 8-wave float16 form: the !LEX instantiation; above 32: bounded passes of 32
    entries, of 20 on the wide float32 form) on the ascending ladder and on plateau 3: r well-separated rungs, then 321
    bit-equal scores - over the k-th place and over every pass boundary (ranks 20, 32, 40, 52, 64).  Expected: the r
    rungs, then the lowest plateau indices."""
    sp = spacing_of(form, f16_spacing)
    with Engine(monkeypatch, form) as eng:
        for keep_n in KEEP_NS:
            case, perm = ordered(MID, 70, "ascending", "ncc", sp)
            s, i, cnt = eng.sweep(case.exp, case.dic, "ncc", keep_n)
            record(eng, "ladder ascending", MID, keep_n, cnt)
            check(eng, case, case.exp, s, i, keep_n)
            for r in {min(12, keep_n - 1), min(25, keep_n - 1)}:
                case = plateau_case(MID, "scattered", r, sp)
                s, i, cnt = eng.sweep(case.exp, case.dic, "ncc", keep_n)
                record(eng, f"plateau 3, r = {r}", MID, keep_n, cnt)
                check(eng, case, case.exp, s, i, keep_n)
                assert np.all(bits(s[:, r:]) == bits(s[:, r:r + 1])), "the plateau's scores are not bit-equal"


@pytest.mark.parametrize("form", list(FORMS))
def test_plateaus_longer_than_the_candidate_buffers(monkeypatch, form, f16_spacing):
    """Plateaus 1, 2 and 4: an all-identical dictionary (pushed at a non-zero start index), 321 copies of the best rung
    in one run and scattered over every tile, and 300 degenerate patterns above an all-negative ladder: the lowest
    indices, and for the last one the score +0.0 exactly (sign bit clear)."""
    sp = spacing_of(form, f16_spacing)
    with Engine(monkeypatch, form) as eng:
        for size in (MID, SMALL):
            for keep_n in (20, 40):
                case = plateau_case(size, "identical")
                s, i, cnt = eng.sweep(case.exp_u8, case.dic, "ncc", keep_n, start=5000)
                record(eng, "plateau 1", size, keep_n, cnt)
                assert np.array_equal(i, np.tile(5000 + np.arange(keep_n), (size[0], 1)))
                check(eng, case, case.exp_u8, s, i, keep_n, start=5000)
                assert np.all(bits(s) == bits(s[:, :1]))
                for kind in ("contiguous", "scattered"):
                    case = plateau_case(size, kind, 0, sp)
                    s, i, cnt = eng.sweep(case.exp, case.dic, "ncc", keep_n, push="three" if kind == "scattered" else "one")
                    record(eng, "plateau 2 " + kind, size, keep_n, cnt)
                    check(eng, case, case.exp, s, i, keep_n)
                    assert np.all(bits(s) == bits(s[:, :1]))
                case = plateau_case(size, "zeros")
                s, i, cnt = eng.sweep(case.exp, case.dic, "ncc", keep_n)
                record(eng, "plateau 4", size, keep_n, cnt)
                check(eng, case, case.exp, s, i, keep_n)
                assert np.all(s == 0) and not np.signbit(s).any(), "degenerate patterns must score +0.0"


@pytest.mark.parametrize("form", list(FORMS))
def test_push_patterns(monkeypatch, form, f16_spacing):
    """One push, three uneven chunks (the bound persists across them), chunks of 700 (they coalesce), a non-zero start
    index, 8 shards merged on the host: the same lists bit for bit, on the ascending ladder and on plateau 3."""
    sp = spacing_of(form, f16_spacing)
    with Engine(monkeypatch, form) as eng:
        for keep_n in (20, 40):
            for label, case in (("ladder ascending", ordered(MID, 70, "ascending", "ncc", sp)[0]),
                                ("plateau 3, r = 12", plateau_case(MID, "scattered", 12, sp))):
                ref = None
                for push, start in (("one", 0), ("three", 0), ("small", 0), ("one", 3001), ("shards", 0)):
                    if push == "shards" and eng.compute == F64:
                        continue   # (float64 lists are merged by the ranks' gather, not from float32 exports)
                    s, i, cnt = eng.sweep(case.exp_u8, case.dic, "ncc", keep_n, push, start)
                    record(eng, label, MID, keep_n, cnt, push=push, start=start)
                    check(eng, case, case.exp_u8, s, i, keep_n, start=start)
                    if ref is None:
                        ref = (bits(s), i)
                    else:
                        assert np.array_equal(i - start, ref[1]) and np.array_equal(bits(s), ref[0]), (push, start)


def test_f32_forms_agree_bit_for_bit(monkeypatch):
    """match.hip == the wide form == its tail variants == natural tile order, and profiling level 3 == none, on hostile
    orders and plateaus."""
    cases = [("ladder ascending", ordered(LARGE, 20, "ascending")[0], 20), ("ladder last_rows", ordered(MID, 20, "last_rows")[0], 20),
             ("plateau 3", plateau_case(MID, "scattered", 25), 40), ("plateau 2", plateau_case(MID, "contiguous", 0), 20)]
    ref = {}
    for form in F32_FORMS:
        for prof in (None, "epilogue"):
            if prof and not FORMS[form][3]:
                continue
            with Engine(monkeypatch, form, prof) as eng:
                for label, case, keep_n in cases:
                    s, i, _ = eng.sweep(case.exp, case.dic, "ncc", keep_n)
                    if label not in ref:
                        ref[label] = (bits(s), i)
                        check(eng, case, case.exp, s, i, keep_n)
                    else:
                        assert np.array_equal(i, ref[label][1]), (form, prof, label)
                        assert np.array_equal(bits(s), ref[label][0]), (form, prof, label)


BUFFERED = [f for f, v in FORMS.items() if v[3]]


@pytest.mark.parametrize("form", BUFFERED)
def test_the_slow_paths_really_ran(monkeypatch, form, f16_spacing):
    """Profiling level 3 counts what the epilogues of match16.hip did.  A chunk is swept as ONE launch here
    (KPDI_UPLOAD_TILES: the upload pipeline may cut it into launches of a tile or two per workgroup, each with fresh buffers).

    Grouped plan (4 096 patterns x 28 300 entries: 110 whole tiles over 16 splits, 64 lists per pattern, 96-entry buffers).
    Under natural tile order a rising dictionary makes every entry of a workgroup's next tile a candidate - 32 per lane and
    tile with two grains - so a buffer overflows on the workgroup's fifth tile at the latest.  Plateau 1 does the same under
    either tile order: a tie passes the non-strict threshold.  Plateau 2 need NOT overflow these buffers, from the code: a lane
    sees 64 rows of a tile, the 321 copies of one run lie in two neighbouring tiles, and the static hand-out (tiles sp, sp +
    nsplit, ...) gives those to different workgroups - at most 64 more candidates for a 96-entry buffer, which overflows only
    where it held over 32 already (measured: 3 ... 6 events of 65 536 lists; scattered, a lane sees about one copy per tile:
    none).  It is recorded there and asserted where it must overflow:

    Plain plan (16 384 patterns x 1 800 entries: 64 row blocks x 4 splits of 2 tiles, 16 lists per pattern < keep_n = 20, so
    bound_rank = 2 and 8-entry buffers).  A workgroup's first tile builds its lists directly (counted as first_tiles_direct),
    its second one overflows on the rising ladders (fewer than 3 rounds: no permutation, whatever KPDI_TILE_ORDER says) and
    on plateau 2 (scattered: 320 copies in 1 800 rows are ~11 of the 64 rows a lane sees in a tile).  Plateau 1 CANNOT
    overflow here, from the code: the first tile leaves a BUILT list of 20 equal scores, and a tie with a built list's last
    entry is appended only with a lower index (`v > last[cg] || idx < lidx[cg]`) - the second tile's indices are all higher,
    nothing is appended (measured: 0 per list).  On the grouped plan the lists are not built yet, so every tie is.

    Late plateau (grouped plan): an all-identical dictionary behind one, two or three whole rounds (16 splits x 256 entries
    each) of lower scores.  Under the permuted walk (6 rounds, stride 5: round slots 0, 5, 4, 3, 2, 1) a workgroup meets the
    winning ties AFTER higher-index ties have filled and overflowed its buffers, one of the three on the very tile that
    overflows - where `scan16` must admit a tie with the list's last entry (non-strict threshold under LEX) and rank it by
    index.  Expected: the plateau's lowest indices.

    Under the PERMUTED order the rising ladders of the grouped plan are recorded, not asserted: the permutation exists to keep
    them from overflowing.  The counters exist only in the LEX instantiations (match16.hip: `if (LEX && a.epi_stats)`),
    which keep_n = 20 selects in every form; the 32-entry lists of the 8-wave float16 form (!LEX) are covered by the exact
    expectations of the keep_n = 32 cases above instead."""
    sp = spacing_of(form, f16_spacing)
    natural = FORMS[form][1].get("KPDI_TILE_ORDER") == "natural"
    with Engine(monkeypatch, form, "epilogue", {"KPDI_UPLOAD_TILES": "4096"}) as eng:
        for size, plan in ((LARGE, "grouped"), (PLAIN, "plain, rank 2")):
            for name in ("shuffled", "ascending", "block_ascending"):
                case, perm = ordered(size, 20, name, "ncc", sp)
                s, i, cnt = eng.sweep(case.exp_u8, case.dic, "ncc", 20)
                rec = record(eng, "ladder " + name, size, 20, cnt)
                check(eng, case, case.exp_u8, s, i, 20)
                assert rec["bound_plan"] == plan, rec
                if name != "shuffled" and (natural or size is PLAIN):
                    assert cnt["epi_overflows"] > 0, rec
            for kind in ("identical", "contiguous", "scattered"):
                case = plateau_case(size, kind, 0, sp)
                s, i, cnt = eng.sweep(case.exp, case.dic, "ncc", 20)
                rec = record(eng, "plateau 1" if kind == "identical" else "plateau 2 " + kind, size, 20, cnt)
                check(eng, case, case.exp, s, i, 20)
                if kind == "identical" and size is LARGE:
                    for rounds in (1, 2, 3):
                        late = plateau_case(size, "late", rounds * 16 * 256)
                        s, i, c2 = eng.sweep(late.exp, late.dic, "ncc", 20)
                        rec2 = record(eng, f"plateau 1 behind {rounds} round(s)", size, 20, c2)
                        check(eng, late, late.exp, s, i, 20)
                        assert c2["epi_overflows"] > 0, rec2
                if (kind == "identical") == (size is LARGE):
                    assert cnt["epi_overflows"] > 0, rec
                elif kind == "identical":
                    assert cnt["epi_appended"] == 0, rec
