"""The merge case tables of tests/_merge_cases.py without a GPU: csrc/merge_plan.h compiled with the host compiler (the
plan's boundaries, the division-free list index), closure of the table over the kernels' forks, the references against
plain restatements and the oracle's merge, and the condition that keeps the GPU test sharp: four deliberately wrong merges
each change the expected output of some case in every cell where that fault can occur."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _merge_cases as M
from conftest import ROOT
from oracle import kpdi_oracle as ko

PLAN_PROBE = r"""
#include "merge_plan.h"
#include <cstdio>
#include <cstring>
int main(int argc, char **argv) {
  using namespace kpdi;
  if (argc > 1 && !std::strcmp(argv[1], "index")) {
    long bad = 0;
    for (int len = 1; len <= 1024; ++len)
      for (int local = 0; local < 16384; ++local) bad += merge_list_index(local, len) != local / len;
    std::printf("%ld\n", bad);
    return 0;
  }
  int n;
  while (std::scanf("%d", &n) == 1) {
    const MergePlan p = merge_plan(n);
    std::printf("%d %d %d %d %d\n", p.id, p.family, p.nk, p.capacity, p.family == MERGE_CACHED ? merge_packed_capacity(p.nk) : -1);
  }
  for (int id = -1; id <= MERGE_PLANS; ++id) std::printf("of %d %d\n", id, merge_plan_of(id).id);
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("merge_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


def plans(exe, totals):
    out = subprocess.run([exe], input=" ".join(map(str, totals)), check=True, capture_output=True, text=True).stdout.split("\n")
    return [tuple(map(int, line.split())) for line in out if line and not line.startswith("of")], \
        [tuple(map(int, line.split()[1:])) for line in out if line.startswith("of")]


def test_plan_boundaries(plan_exe):
    totals = [1, 256, 257, 768, 769, 1536, 1537, 3072, 3073, 6144, 6145, 16384, 16385, 20001, 2**31 - 1]
    got, named = plans(plan_exe, totals)
    want = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 6]
    assert [g[0] for g in got] == want
    assert [g[1] for g in got] == [0] * 8 + [1] * 4 + [2] * 3  # cached, block, generic
    assert [g[2] for g in got] == [M.NK[p] for p in want]
    assert [g[3] for g in got] == [M.CAPACITY[p] or 2**31 - 1 for p in want]
    assert [g[4] for g in got[:8]] == [256, 256, 512, 512, 512, 512, 512, 512]
    assert named == [(-1, -1)] + [(i, i) for i in range(7)] + [(7, -1)]
    # the table's own restatement, over every total
    sweep = list(range(1, 20100, 7)) + totals
    assert [g[0] for g in plans(plan_exe, sweep)[0]] == [M.plan_of(n) for n in sweep]
    assert {M.candidates(c) for c in M.CASES} >= set(totals[1:14])


def test_list_index_is_integer_division(plan_exe):
    """Every len in 1..1024 and every local < 16384: len = keep_n reaches the inline, not only the lists' 32."""
    assert subprocess.run([plan_exe, "index"], check=True, capture_output=True, text=True).stdout.strip() == "0"


# ---- closure ------------------------------------------------------------------------------------------------------------
def unreachable(plan, mode, n_src, seg, packed):
    cached = plan.startswith("cached")
    if not cached and mode == "lanes":
        return "one workgroup per pattern / the generic kernel read counts from memory per candidate"
    if cached != (packed is not None):
        return "only the wave-per-pattern kernels pack candidates into LDS"
    if plan == "cached4" and packed is False:
        return "<4> holds 256 candidates and packs up to 256: never unpacked"
    return None


def all_cells():
    return [(p, mode, n, seg, pk) for p in M.PLANS for mode in ("none", "lanes", "memory") for n in (1, 2, 3)
            for seg in (False, True) for pk in (True, False, None)]


@pytest.fixture(scope="module")
def reached():
    out = {}
    for c in M.CASES:
        for cell in M.cells(c):
            out.setdefault(cell, []).append(c)
    return out


def test_case_table(reached):
    assert len(M.CASES) == 122 and {c.m for c in M.CASES} >= {1, 3, 5, 9} and {c.k for c in M.CASES} >= {1, 20, 32, 33, 70}
    assert {c.seg_n for c in M.CASES} == {0, 1, 2, 16}
    assert {s.len for c in M.CASES for s in c.srcs if not (s.lists == 1 and s.len == c.k) and not s.gather} == {1, 8, 20, 32}
    listed = [cell for cell in all_cells() if unreachable(*cell)]
    for cell in listed:
        assert cell not in reached, (cell, unreachable(*cell), reached[cell][0].name)
    missing = [cell for cell in all_cells() if not unreachable(*cell) and cell not in reached]
    assert not missing, missing
    assert len(all_cells()) - len(listed) == 18 * (1 + 3 * 2) + 12 * 3 == 162  # <4> packed, <12 | 24 | 48> both; two counts modes for the other three
    # real candidates either side of each packing limit, thinned by counts and by INT_MAX entries
    for name, limit, total in (("nk4", 256, 256), ("nk12", 512, 768)):
        for thin in ("counts", "intmax"):
            got = {M.n_real(c, M.build(c), 0) for c in M.CASES if c.name.startswith(f"real-{name}-") and c.thin == thin}
            assert got == {0, 1, limit - 1, limit, min(limit + 1, total), total}, (name, thin, got)
    for c in M.CASES:
        b = M.build(c)
        for s, lay in zip(c.srcs, b.sources):  # every extent inside its buffer
            assert (c.m - 1) * lay["row_stride"] + (s.lists - 1) * lay["list_stride"] + s.len <= lay["scores"].size
        if c.real is not None:
            assert {M.n_real(c, b, mi) for mi in range(c.m)} == {c.real}, c.name
    # poison behind the counts: every counted case has entries there, all of them winners if read
    for c in M.CASES:
        if any(s.counted for s in c.srcs) and c.real is None:
            b = M.build(c)
            extra = [len(M.entries(c, b, mi, ignore_counts=True)[0]) - M.n_real(c, b, mi) for mi in range(c.m)]
            assert max(extra) > 0, c.name


def test_reference_against_lexsort_and_the_oracle():
    for c in M.CASES:  # what the table promises of EVERY case: distinct (score, index) pairs - indeed distinct indices - no NaN
        b = M.build(c)
        for mi in range(c.m):
            s, i = M.entries(c, b, mi)
            assert len(set(i.tolist())) == len(i) and not np.isnan(s).any(), (c.name, mi)
    for c in M.CASES[::3]:
        b = M.build(c)
        want_s, want_i = M.reference(c, b)
        for mi in range(c.m):
            s, i = M.entries(c, b, mi)
            pairs = sorted(zip((-(s + np.float32(0)).astype(np.float64)).tolist(), i.tolist()))[: c.k]
            pairs += [(np.inf, M.INT_MAX)] * (c.k - len(pairs))
            cols = slice(c.out_offset, c.out_offset + c.k)
            assert [(float(a), int(j)) for a, j in zip(want_s[mi, cols], want_i[mi, cols])] == [(-p[0], p[1]) for p in pairs]
            assert not np.signbit(want_s[mi, cols][want_s[mi, cols] == 0]).any()
            rest = np.ones(M.out_stride(c), bool)
            rest[cols] = False
            assert (want_s[mi, rest] == M.SENTINEL_S).all() and (want_i[mi, rest] == M.SENTINEL_I).all()
    # the oracle's merge: running best-k + one chunk's best, no counts, no holes
    c = M.Case("oracle", 5, 20, (M.Src(1, 20), M.Src(1, 32)), real=52, thin="intmax", order="plain")
    b = M.build(c)
    run, chunk = b.sources
    got = ko.merge_topk(run["scores"].reshape(5, 20), run["idx"].reshape(5, 20), chunk["scores"].reshape(5, 32),
                        chunk["idx"].reshape(5, 32), 20)
    want = M.reference(c, b)
    assert np.array_equal(got[0] + np.float32(0), want[0]) and np.array_equal(got[1], want[1])


def test_reference_equals_the_order_of_the_kernels_keys():
    """merge.hip's topk_key restated: the distinct 64-bit keys of a pattern's entries, largest first, decoded again, are
    the reference's rows - for every case (so nothing in the table leans on a pair the key order would collapse)."""
    def keys(s, i):
        u = (s + np.float32(0)).view(np.uint32).astype(np.uint64)
        u = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
        return (u << np.uint64(32)) | (M.INT_MAX - i).astype(np.uint64)

    for c in M.CASES:
        b = M.build(c)
        want_s, want_i = M.reference(c, b)
        for mi in range(c.m):
            k = np.unique(keys(*M.entries(c, b, mi)))[::-1][: c.k]
            assert (k != 0).all()
            u = (k >> np.uint64(32)).astype(np.uint32)
            u = np.where(u & 0x80000000, u ^ 0x80000000, ~u).astype(np.uint32)
            got_s, got_i = np.full(c.k, -np.inf, np.float32), np.full(c.k, M.INT_MAX, np.int64)
            got_s[: len(k)] = u.view(np.float32)
            got_i[: len(k)] = M.INT_MAX - (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
            cols = slice(c.out_offset, c.out_offset + c.k)
            assert np.array_equal(got_s.view(np.uint32), want_s[mi, cols].view(np.uint32)), (c.name, mi)
            assert np.array_equal(got_i, want_i[mi, cols]), (c.name, mi)


FAULTS = {
    "counts ignored": (dict(ignore_counts=True), lambda cell: cell[1] != "none"),
    "ties broken by memory order": (dict(memory_ties=True), lambda cell: True),
    "segments not applied": (dict(no_segments=True), lambda cell: cell[3]),
    "last slot of the last list dropped": (dict(drop_last=True), lambda cell: True),
}


@pytest.mark.parametrize("fault", FAULTS)
def test_a_wrong_merge_changes_the_expected_output_in_every_cell(fault, reached):
    kw, possible = FAULTS[fault]
    changed = {}
    for c in M.CASES:
        b = M.build(c)
        right, wrong = M.reference(c, b), M.reference(c, b, **kw)
        changed[c.name] = not (np.array_equal(right[0].view(np.uint32), wrong[0].view(np.uint32)) and
                               np.array_equal(right[1], wrong[1]))
    blind = [cell for cell, cs in reached.items() if possible(cell) and not any(changed[c.name] for c in cs)]
    assert not blind, (fault, blind)


# ---- float64 merge and fill ---------------------------------------------------------------------------------------------
def test_f64_table():
    names = [c.name for c in M.CASES64]
    assert len(set(names)) == len(names)
    for c in M.CASES64:
        s, i, unc = M.reference64(c)
        n = (c.k if c.run else 0) + c.lists * c.len
        for mi in range(c.m):
            es, ei = M.entries64(c, mi)
            want = sorted(zip((-es).tolist(), ei.tolist(), range(n)))[: c.k]
            assert [(-a, b) for a, b, _ in want] == list(zip(s[mi, : len(want)].tolist(), i[mi, : len(want)].tolist()))
            assert (s[mi, len(want):] == M.SENTINEL64_S).all()
        if c.cert is not None:  # patterns 0, 2 (mod 4) are built to fail, 1 and 3 to pass
            assert unc == (0 if c.cert["enumerated_all"] else c.m // 2), c.name
    by = {c.name: c for c in M.CASES64}
    assert by["fewer-than-k"].lists * by["fewer-than-k"].len < by["fewer-than-k"].k and not by["fewer-than-k"].run
    lds = lambda c: ((c.k if c.run else 0) + c.lists * c.len) * 12
    assert lds(by["lds-64k"]) <= 64 * 1024 < lds(by["lds-over-64k"]) and lds(by["lds-150k"]) == 150 * 1024 < lds(M.LDS_REFUSED)
    assert any(len(set(zip(*M.entries64(by["plain"], mi)))) < 44 for mi in range(5))  # identical pairs occur


def test_fill_table():
    assert max(len(r) for r in M.FILL_LAUNCHES.values()) == 8
    used, paths = set(), set()
    for name, ranges in M.FILL_LAUNCHES.items():
        spans = sorted((off // 4, off // 4 + n) for off, n, _, _ in ranges)
        assert spans[0][0] >= 16 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), name
        ref = M.fill_reference(ranges)
        touched = np.zeros(ref.size, bool)
        for a, b in spans:
            touched[a:b] = True
        assert (ref[~touched] == M.GUARD).all() and (ref[touched] != M.GUARD).all() and (~touched[-16:]).all()
        for off, n, _, u in ranges:
            used.add(u)
            paths.add((u < 0, off % 16 == 0 and n % 4 == 0, n == 0))
    assert used >= {-1, 0, 1, 31, 32}
    assert paths >= {(True, True, False), (True, False, False), (True, True, True), (False, True, False), (False, False, False)}
