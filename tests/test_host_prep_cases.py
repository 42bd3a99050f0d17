"""The pixel-probe case table of tests/_prep_cases.py without a GPU: csrc/prep_plan.h compiled with the host compiler says
which preparation kernel every case runs (closure: every reachable kernel family x operand form x masked / unmasked x
metric is met), the plan's arithmetic at its boundaries, the float64 reference against the oracle, the probes' positions,
and the condition that keeps the GPU test sharp: a probe moved to the adjacent kept pixel changes its scores by far more
than the tolerance."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _prep_cases as P
from conftest import ROOT
from kikuchipy_amd import _lib
from oracle import kpdi_oracle as ko

KERNELS = ("GENERIC", "WAVE1", "WAVE4", "WAVE_LINES", "WAVE_MASKED", "WAVE_MASKED_DMA", "WAVE_GATHER", "BLOCK",
           "BLOCK_MASKED", "PREP32_BLOCK4", "PREP16_BLOCK4")
FIELDS = ("kernel h16 masked lines np pass_form grid threads lds split_after span wave_path block_path vec_ok vec4 staged "
          "staged_dma gather block_vec block_masked have_desc").split()

PLAN_PROBE = r"""
#include "prep_plan.h"
#include <cstdio>
#include <map>
int main() {
  std::map<int, std::vector<int>> maps;
  char tag;
  while (std::scanf(" %c", &tag) == 1) {
    if (tag == 'M') {
      int id, k;
      std::scanf("%d %d", &id, &k);
      std::vector<int> m(k);
      for (int &p : m) std::scanf("%d", &p);
      maps[id] = m;
      continue;
    }
    int dtype, npix, k, kpad, metric, form, map_id, n_out, ns, nl, nd, ng, p16;
    unsigned long long addr;
    std::scanf("%d %d %d %d %d %d %d %llu %d %d %d %d %d %d", &dtype, &npix, &k, &kpad, &metric, &form, &map_id, &addr,
               &n_out, &ns, &nl, &nd, &ng, &p16);
    bool desc = false;
    if (map_id >= 0) {
      std::vector<unsigned> d;
      desc = kpdi::gather_descriptors(maps[map_id].data(), k, npix, &d);
    }
    kpdi::PrepSwitches sw;
    sw.no_staged = ns, sw.no_lines = nl, sw.no_dma = nd, sw.no_gather = ng, sw.prep16 = p16;
    const kpdi::PrepPlan p = kpdi::prep_plan(dtype, npix, k, kpad, metric, form, map_id >= 0, desc, addr, n_out, sw);
    std::printf("%d %d %d %d %d %d %u %u %zu %d %d %d %d %d %d %d %d %d %d %d %d\n", p.kernel, p.h16, p.masked, p.lines, p.np,
                p.pass_form, p.grid, p.threads, p.lds_bytes, p.split_after, p.span, p.wave_path, p.block_path, p.vec_ok,
                p.vec4, p.staged, p.staged_dma, p.gather, p.block_vec, p.block_masked, (int)desc);
  }
}
"""


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("prep_plan")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PLAN_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "kikuchipy_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    return str(exe)


def round_up(v, m):
    return -(-v // m) * m


def kpad_of(k, metric, form):
    """api.hip: set_detector_layout / sweep.hip: decide_form."""
    if form == 2:
        return round_up(k, 48) // 2
    return round_up(k + (metric == "ndp"), 24 if form == 3 else 32)


def launches(c, side):
    """The two launch_prep calls of a case's side as prep_plan arguments: (experimental set, dictionary chunk)."""
    form = P.FORMS[c.compute]
    b_n = c.n - 2 if (c.nav and c.n > 3 and side == "b") else c.n
    nprobes = len(P.probe_list(c.shape, c.mask))
    k = len(P.kept_pixels(c.shape, c.mask))
    metric = {"ncc": 0, "ndp": 1 if form == 2 else 2}[c.metric]
    es = np.dtype(c.dtype).itemsize
    offset = {"dev1": es, "devb4": 4, "devb8": 8, "devb12": 12}.get(c.push, 0)
    exp_dtype, dic_dtype = ("float32", c.dtype) if side == "a" else (c.dtype, "float32")
    env = dict(c.env)
    sw = [int("KPDI_PREP_NO_" + s in env) for s in ("STAGED", "LINES", "DMA", "GATHER")]
    sw.append({"block": 1, "block4": 2}.get(env.get("KPDI_PREP16"), 0))
    common = dict(npix=c.shape[0] * c.shape[1], k=k, kpad=kpad_of(k, c.metric, form), metric=metric, form=form,
                  mask=(c.shape, c.mask) if c.mask != "none" else None, sw=sw)
    return (dict(common, dtype=exp_dtype, addr=0, n_out=nprobes if side == "a" else b_n),  # (exp_raw is an allocation of its own)
            dict(common, dtype=dic_dtype, addr=offset if side == "a" else 0, n_out=c.n if side == "a" else nprobes))


def evaluate(exe, items):
    """prep_plan of every launch in `items` (dicts as `launches` makes them) -> list of dicts of FIELDS."""
    ids, lines = {}, []
    for it in items:
        m = it["mask"]
        if m is not None and m not in ids:
            ids[m] = len(ids)
            keep = P.kept_pixels(*m)
            lines.append(f"M {ids[m]} {len(keep)} " + " ".join(map(str, keep)))
        lines.append("L {} {} {} {} {} {} {} {} {} {}".format(
            _lib.DTYPE_CODES[np.dtype(it["dtype"])] if not isinstance(it["dtype"], int) else it["dtype"], it["npix"], it["k"],
            it["kpad"], it["metric"], it["form"], ids[m] if m is not None else -1, it["addr"], it["n_out"],
            " ".join(map(str, it["sw"]))))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout.split("\n")
    plans = [dict(zip(FIELDS, map(int, line.split()))) for line in out if line]
    assert len(plans) == len(items)
    return plans


def name(plan):
    return KERNELS[plan["kernel"]]


@pytest.fixture(scope="module")
def table_plans(plan_exe):
    items, owners = [], []
    for c in P.CASES:
        for side in "ab":
            for it in launches(c, side):
                items.append(it)
                owners.append((c, side))
    return list(zip(owners, items, evaluate(plan_exe, items)))


def test_case_count():
    assert len(P.CASES) == 502 and len({P.case_id(c) for c in P.CASES}) == len(P.CASES)
    assert {c.dtype for c in P.CASES} == set(P.DTYPES) and {c.n for c in P.CASES} == {1, 37, 69}
    assert {c.push for c in P.CASES} == {"host", "dev0", "dev1", "devb4", "devb8", "devb12", "held"}
    for compute in P.FORMS:
        assert any(c.push == "held" and c.compute == compute for c in P.CASES)
        assert {c.shape for c in P.CASES if c.compute == compute} >= set(P.FORM2_TOLERANCES)
    assert {k for c in P.CASES for k, _ in c.env} == {"KPDI_PREP_NO_STAGED", "KPDI_PREP_NO_LINES", "KPDI_PREP_NO_DMA",
                                                      "KPDI_PREP_NO_GATHER", "KPDI_PREP16"}


# cells (kernel, operand form, masked, metric) that no input reaches, each with its reason; every other cell is met
def unreachable(kernel, form, masked):
    if kernel in ("WAVE4", "WAVE_LINES", "BLOCK") and masked:
        return "vector loads straight to registers: only without a pixel map"
    if kernel in ("WAVE_MASKED", "WAVE_MASKED_DMA", "WAVE_GATHER", "BLOCK_MASKED") and not masked:
        return "gathers through the pixel map: only with a signal mask"
    if kernel == "WAVE_LINES" and form < 2:
        return "whole lines of the plane-major layouts: forms 2 and 3 only"
    if kernel in ("BLOCK", "BLOCK_MASKED") and form == 3:
        return "form 3 sends every workgroup-per-pattern launch to prep32_block4_kernel"
    if kernel == "PREP32_BLOCK4" and form != 3:
        return "writes the wide float32 layout: form 3 only"
    if kernel == "PREP16_BLOCK4" and form != 2:
        return "writes the float16 layout: form 2 only"
    return None


def test_plan_closure(table_plans, plan_exe):
    reached = {}
    for (c, side), it, p in table_plans:
        reached.setdefault((name(p), it["form"], it["mask"] is not None, c.metric), P.case_id(c) + "/" + side)
    cells = [(k, f, m, me) for k in KERNELS for f in range(4) for m in (False, True) for me in P.METRICS]
    listed = {cell: unreachable(*cell[:3]) for cell in cells if unreachable(*cell[:3])}
    assert len(listed) == 2 * 44, len(listed)
    for cell, why in listed.items():
        assert cell not in reached, f"{cell} is listed as unreachable ({why}) but {reached.get(cell)} reaches it"
    missing = [cell for cell in cells if cell not in listed and cell not in reached]
    assert not missing, missing
    # the listed cells stay unreachable over a wide sweep of plan inputs, switches included
    items = []
    for dtype in ("uint8", "float32", "float64"):
        for (sy, sx) in ((24, 20), (45, 45), (60, 60), (64, 65), (90, 91), (128, 128), (150, 150)):
            for mask in ("none", "crop", "scatter"):
                for form in range(4):
                    for sw in ([0, 0, 0, 0, 0], [1, 0, 0, 0, 1], [0, 1, 1, 0, 2], [0, 0, 1, 1, 0], [1, 1, 1, 1, 1]):
                        for addr in (0, 4):
                            k = len(P.kept_pixels((sy, sx), mask))
                            items.append(dict(dtype=dtype, npix=sy * sx, k=k, kpad=kpad_of(k, "ncc", form), metric=0,
                                              form=form, mask=None if mask == "none" else ((sy, sx), mask), addr=addr,
                                              n_out=37, sw=sw))
    for it, p in zip(items, evaluate(plan_exe, items)):
        assert unreachable(name(p), it["form"], it["mask"] is not None) is None, (it, name(p))


def test_every_dtype_meets_every_family_in_forms_0_and_3(table_plans):
    met = {}
    for (c, side), it, p in table_plans:
        met.setdefault((name(p), it["form"]), set()).add(str(np.dtype(it["dtype"])))
    for form, kernels in ((0, ("GENERIC", "WAVE1", "WAVE4", "WAVE_MASKED", "BLOCK", "BLOCK_MASKED")),
                          (3, ("GENERIC", "WAVE1", "WAVE_LINES", "WAVE_MASKED", "PREP32_BLOCK4"))):
        for k in kernels:
            assert met[(k, form)] >= set(P.DTYPES), (k, form, set(P.DTYPES) - met[(k, form)])
        for k in ("WAVE_MASKED_DMA", "WAVE_GATHER"):  # float32 rows only
            assert met[(k, form)] == {"float32"}
    top = {(name(p), it["form"]) for (c, side), it, p in table_plans if c.variant == "top" and it["dtype"] == c.dtype}
    assert len(top) >= 10


def test_switches_and_offsets_change_the_plan(plan_exe):
    """Every case with a switch or an offset pointer runs another kernel (or geometry) than the same case without."""
    n = 0
    for c in P.CASES:
        if not c.env and c.push in ("host", "dev0", "held"):
            continue
        base = c._replace(env=(), push="host")
        a, b = evaluate(plan_exe, [launches(c, "a")[1], launches(base, "a")[1]])
        if c.push.startswith("devb") and name(b) == "WAVE_GATHER":
            assert name(a) == "WAVE_GATHER"  # needs 4-byte alignment only: the same kernel from an odd base
        else:
            assert (name(a), a["np"]) != (name(b), b["np"]), P.case_id(c)
        n += 1
    assert n > 60


def test_identity_pairs_differ_only_in_how_bytes_are_loaded(plan_exe):
    same_sums = [{"WAVE_GATHER", "WAVE_MASKED_DMA", "WAVE_MASKED"}, {"WAVE_LINES", "WAVE4"}, {"PREP16_BLOCK4"}]
    met = set()
    for x, y in P.IDENTITY_PAIRS:
        assert P.patterns(x).tobytes() == P.patterns(y).tobytes()
        for side in "ab":
            for px, py in zip(evaluate(plan_exe, launches(x, side)), evaluate(plan_exe, launches(y, side))):
                assert any(name(px) in s and name(py) in s for s in same_sums), (P.case_id(x), P.case_id(y), name(px), name(py))
                met.add((name(px), name(py), px["np"], py["np"]))
    assert {("WAVE_GATHER", "WAVE_MASKED_DMA", 0, 0), ("WAVE_GATHER", "WAVE_MASKED", 0, 0), ("WAVE_MASKED_DMA", "WAVE_MASKED", 0, 0),
            ("WAVE_LINES", "WAVE4", 0, 0), ("PREP16_BLOCK4", "PREP16_BLOCK4", 2, 4), ("WAVE_GATHER", "WAVE_GATHER", 0, 0)} <= met


def test_plan_arithmetic(plan_exe):
    def plan(k, form, metric="ncc", dtype="uint8", npix=None, mask=None, addr=0, n_out=37, sw=(0, 0, 0, 0, 0)):
        m = {"ncc": 0, "ndp": 1 if form == 2 else 2}[metric]
        return evaluate(plan_exe, [dict(dtype=dtype, npix=npix or k, k=k, kpad=kpad_of(k, metric, form), metric=m, form=form,
                                        mask=mask, addr=addr, n_out=n_out, sw=list(sw))])[0]

    # one wave per pattern up to a span of 4096 columns, one workgroup up to 16 384, the generic kernel beyond
    for form in (0, 1):
        assert name(plan(4096, form)) == "WAVE4" and plan(4096, form)["span"] == 4096
        assert name(plan(4100, form)) == "BLOCK" and name(plan(4097, form, npix=4097)) == "GENERIC"  # (K % 4)
        assert name(plan(16384, form)) == "BLOCK" and name(plan(16388, form)) == "GENERIC"
        # ndp: the extra column is padding's first, until K fills its last slab
        assert name(plan(4092, form, "ndp")) == "WAVE4" and name(plan(4096, form, "ndp")) == "BLOCK"
        assert name(plan(16384, form, "ndp")) == "GENERIC" and plan(16384, form, "ndp")["span"] == 16416
    # form 3 pads to 24 columns, form 2 to 48 pixels (kpad counts pairs: span = 2 * kpad)
    assert name(plan(4080, 3)) == "WAVE_LINES" and plan(4096, 3)["span"] == 4104 and name(plan(4096, 3)) == "PREP32_BLOCK4"
    assert name(plan(16368, 3)) == "PREP32_BLOCK4" and name(plan(16384, 3)) == "GENERIC"
    assert name(plan(4080, 3, "ndp")) == "PREP32_BLOCK4" and name(plan(4076, 3, "ndp")) == "WAVE_LINES"
    assert name(plan(4080, 2)) == "WAVE_LINES" and plan(4080, 2)["span"] == 4080
    assert plan(4096, 2)["span"] == 4128 and name(plan(4096, 2)) == "PREP16_BLOCK4" and plan(4096, 2)["np"] == 2
    assert name(plan(16368, 2)) == "PREP16_BLOCK4" and name(plan(16384, 2)) == "GENERIC"
    assert name(plan(4080, 2, "ndp")) == "WAVE_LINES"  # the float16 form carries no extra column
    # grids: four patterns per workgroup on the wave path, persistent workgroups under a mask, 16-unit blocks for NP = 2
    assert plan(3600, 0, n_out=37)["grid"] == 10 and plan(8192, 0, n_out=37)["grid"] == 37
    assert plan(8192, 2, n_out=37)["grid"] == 32 and plan(8192, 2, n_out=37)["threads"] == 512
    p4 = plan(8192, 2, n_out=37, sw=(0, 0, 0, 0, 2))
    assert (p4["grid"], p4["threads"], p4["np"], p4["lds"]) == (10, 1024, 4, 4 * (2 * 4104 + 8) * 2)
    assert plan(8192, 3, n_out=37)["grid"] == 10 and plan(8192, 3)["threads"] == 1024
    assert name(plan(8192, 2, sw=(0, 0, 0, 0, 1))) == "BLOCK" and plan(8192, 2, n_out=37, sw=(0, 0, 0, 0, 1))["grid"] == 64
    big = plan(2867, 0, npix=4096, mask=((64, 64), "scatter"), n_out=100000)
    k = len(P.kept_pixels((64, 64), "scatter"))
    big = plan(k, 0, npix=4096, mask=((64, 64), "scatter"), n_out=100000)
    assert name(big) == "WAVE_MASKED" and big["grid"] == 2048 and big["lds"] == (round_up(k, 4) + 4 * 4096) * 4 > 64 * 1024
    dma = plan(k, 0, dtype="float32", npix=4096, mask=((64, 64), "scatter"), n_out=100000)
    assert name(dma) == "WAVE_MASKED_DMA" and dma["grid"] == 1024 and dma["lds"] == (round_up(k, 4) + 8 * 4096) * 4
    # dynamic LDS stays under the 160 KB of a CU wherever a kernel asks for more than the default 64 KB
    for k in (16368, 16384):
        for form in (2, 3):
            for sw in ((0, 0, 0, 0, 0), (0, 0, 0, 0, 2)):
                p = plan(k, form, sw=sw)
                assert p["lds"] <= 160 * 1024, (k, form, p)
    assert plan(16368, 3)["lds"] == 4 * (8 * ((16368 // 8 + 1) // 2) + 4) * 4 > 64 * 1024
    assert plan(16368, 2, sw=(0, 0, 0, 0, 2))["lds"] == 4 * (16368 + 8) * 2 > 64 * 1024
    # the split-f16 conversion follows only the kernels that store single floats
    assert plan(4097, 1, npix=4097)["split_after"] and plan(2025, 1)["split_after"] and not plan(3600, 1)["split_after"]
    assert not plan(2025, 0)["split_after"] and not plan(8192, 1)["split_after"]
    # alignment: four elements for the vector paths, four bytes for the gather
    assert name(plan(3600, 0, dtype="float64", addr=16)) == "WAVE1" and name(plan(3600, 0, dtype="float64", addr=32)) == "WAVE4"
    assert name(plan(3600, 0, dtype="uint16", addr=2)) == "WAVE1" and name(plan(3600, 0, dtype="uint16", addr=8)) == "WAVE4"
    kc = len(P.kept_pixels((60, 60), "crop"))
    for addr, want in ((0, "WAVE_GATHER"), (4, "WAVE_GATHER"), (12, "WAVE_GATHER"), (2, "WAVE1")):
        assert name(plan(kc, 0, dtype="float32", npix=3600, mask=((60, 60), "crop"), addr=addr)) == want
    assert evaluate(plan_exe, [dict(dtype=99, npix=64, k=64, kpad=64, metric=0, form=0, mask=None, addr=0, n_out=1,
                                    sw=[0] * 5)])[0]["kernel"] == -1


def test_every_lds_request_fits(table_plans):
    for (c, side), it, p in table_plans:
        assert p["lds"] <= 160 * 1024 and p["grid"] >= 1 and p["threads"] in (256, 512, 1024), P.case_id(c)


# ---- the builder -----------------------------------------------------------------------------------------------------
SAMPLE = [c for i, c in enumerate(P.CASES) if i % 13 == 0 and c.shape[0] <= 130]


@pytest.mark.parametrize("c", SAMPLE, ids=P.case_id)
def test_reference_agrees_with_the_oracle(c):
    b = P.build(c)
    for side in "ab":
        exp, dic, nav = P.sides(c, b, side)
        want = P.reference(c, b, side)
        s, i = ko.dictionary_indexing(exp, dic, metric=c.metric, keep_n=len(dic), signal_mask=b.mask, navigation_mask=nav)
        zero = P.zero_entries(c, b, side)
        with np.errstate(invalid="ignore"):
            got = P.assemble(np.nan_to_num(np.asarray(s, dtype=np.float64)), np.asarray(i), len(dic))
        live = ~zero  # (the oracle divides 0 by 0 on degenerate rows; the engine's zero rows are checked on the GPU)
        assert np.abs(got - want)[live].max(initial=0) <= 1e-5
        assert (want[zero] == 0).all()


def test_probes_are_where_they_claim():
    for shape, mask in sorted({(c.shape, c.mask) for c in P.CASES}):
        keep, m = P.kept_pixels(shape, mask), P.signal_mask(shape, mask)
        plist = P.probe_list(shape, mask)
        pats = P.probe_patterns(shape, plist).reshape(len(plist), -1)
        names = [p.name for p in plist]
        assert len(set(names)) == len(names) <= 30
        for p, row in zip(plist, pats):
            assert sorted(np.flatnonzero(row)) == sorted(p.pixels) and [row[q] for q in p.pixels] == list(p.values)
            if p.kind == "kept":
                assert keep[p.kept_index] == p.pixels[0] and row.sum() == 1
            elif p.kind == "out":
                assert m.ravel()[p.pixels[0]] and not row[keep].any()  # all zero under the mask
            else:
                assert len(p.pixels) == 2 and all(q in keep for q in p.pixels)
        K = len(keep)
        for j in P.KEPT_PROBES:
            assert (f"kept{j}" in names) == (j < K) or any(p.kind == "kept" and p.kept_index == j for p in plist)
        assert {p.kept_index for p in plist if p.kind == "kept"} >= set(range(max(K - 5, 0), K))
        if m is not None:
            flat = m.ravel()
            by = {p.name: p for p in plist}
            assert by["out_first"].pixels[0] == np.flatnonzero(flat)[0] and by["out_last"].pixels[0] == np.flatnonzero(flat)[-1]
            q = by["out_beside"].pixels[0]
            assert flat[q] and ((q + 1 < flat.size and not flat[q + 1]) or not flat[q - 1])
            if "rowfirst" in by:
                r = by["rowfirst"].pixels[0] // shape[1]
                cols = np.flatnonzero(~m[r])
                assert 0 < m[r].sum() < shape[1]
                assert by["rowfirst"].pixels[0] == r * shape[1] + cols[0] and by["rowlast"].pixels[0] == r * shape[1] + cols[-1]
        if K >= 2:
            assert sum(p.kind == "double" for p in plist) == 2


@pytest.mark.parametrize("chunk", range(8))
def test_every_case_is_sensitive_to_one_misplaced_pixel(chunk):
    """Moving a kept-pixel probe to the adjacent kept pixel changes at least 90 % of its scores by more than 10 x the
    case's tolerance; degenerate entries (exactly 0 either way) aside."""
    for c in P.CASES[chunk::8]:
        b = P.build(c)
        if len(b.keep) < 2:
            continue
        moved = P.probe_patterns(c.shape, b.plist, displaced=True, kind=c.mask)
        single = np.array([p.kind == "kept" for p in b.plist])
        for side in "ab":
            tol = P.tolerance(c, b, side)
            d = np.abs(P.reference(c, b, side, probes=moved) - P.reference(c, b, side))
            d = (d if side == "a" else d.T)[single]  # (probe, pattern)
            live = P.prepared(b.patterns if b.nav is None or side == "a" else b.patterns[~b.nav], b.keep, c.metric).any(axis=1)
            frac = (d[:, live] > 10 * tol).mean(axis=1)
            assert frac.min() >= 0.9, (P.case_id(c), side, tol, [(p.name, round(float(f), 2)) for p, f in zip([p for p in b.plist if p.kind == "kept"], frac) if f < 0.9])


def test_float16_tolerances():
    worst = {}
    for c in P.CASES:
        if P.FORMS[c.compute] == 2:
            b = P.build(c)
            worst[c.shape] = max(worst.get(c.shape, 0.0), P.tolerance(c, b, "a"), P.tolerance(c, b, "b"))
    print({k: float(f"{v:.2e}") for k, v in sorted(worst.items())})
    assert set(worst) == set(P.FORM2_TOLERANCES)
    for shape, v in worst.items():
        assert 0.9 * P.FORM2_TOLERANCES[shape] <= v <= P.FORM2_TOLERANCES[shape], (shape, v)
