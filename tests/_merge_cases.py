"""Case tables and NumPy references for the merge kernels on their own (csrc/merge.hip, merge64_kernel of
csrc/rescore.hip, fill_segments_kernel): seeded, pure NumPy, no GPU.  tests/test_host_merge_cases.py checks the tables
(which kernel forks they reach, that a wrong merge would change their expected output), tests/test_gpu_merge.py runs them
through kpdi_merge_selftest / kpdi_merge64_selftest / kpdi_fill_selftest and compares bit for bit.

The float32 merge's contract, as `reference` states it: per pattern every entry inside its list's count (all of them
when the source has no counts) whose index is not INT_MAX takes part; the sources in `seg_sources` hold rows, translated
through the segments; the order is (score descending with -0 equal to +0, index ascending); k entries are emitted,
padded with (-inf, INT_MAX); a zero score comes out as +0 (the key adds 0.f); columns outside
[out_offset, out_offset + k) keep what the caller put there.

Two kinds of input are left out on purpose.  (score, index) pairs are distinct within a pattern: the kernels' rounds take
"the largest key strictly below the previous winner", which collapses identical pairs - no caller produces them (a
dictionary index is scored once per pattern).  No score is NaN: the match kernels score degenerate patterns as exactly 0
and never emit NaN.  Everything else a float can be is here: negative scores, +0 and -0, +inf, and -inf with a valid
index (a valid entry that ranks last).

What lies behind a list's count, in the padding between lists and between rows is POISON: score +inf or 3e38 with a
small valid index, which would win every rank if a kernel read one slot too far."""
import functools
from collections import namedtuple

import numpy as np

INT_MAX = 2**31 - 1
PLANS = ("cached4", "cached12", "cached24", "cached48", "block24", "block64", "generic")
NK = (4, 12, 24, 48, 24, 64, 0)
CAPACITY = (256, 768, 1536, 3072, 6144, 16384, None)
CACHED = range(4)
SENTINEL_S, SENTINEL_I = np.float32(7.25), np.int32(-7)  # what the caller prefills the output with

Src = namedtuple("Src", "lists len counted pad_list pad_row gather", defaults=(False, 0, 0, False))
Case = namedtuple("Case", "name m k srcs out_stride out_offset seg_n seg_sources real thin order",
                  defaults=(None, 0, 0, 0, None, "counts", "random"))
Built = namedtuple("Built", "sources segments out_s out_i")


def plan_of(candidates):
    """csrc/merge_plan.h restated (the host test compares it with the compiled header)."""
    for p, cap in enumerate(CAPACITY):
        if cap is None or candidates <= cap:
            return p


def packed_capacity(plan):
    return 64 * min(NK[plan], 8)


def candidates(c):
    return sum(s.lists * s.len for s in c.srcs)


def plans_for(c):
    """Every kernel that can hold the case: the GPU test forces each of them."""
    n = candidates(c)
    return [p for p, cap in enumerate(CAPACITY) if cap is None or n <= cap]


def out_stride(c):
    return c.out_stride or c.k


def seg_mask(c):
    return c.seg_sources if c.seg_n else 0


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2**32)


def _segments(rng, n, slots):
    """n segments over 4 * slots + 64 rows: rows and indices both rise from segment to segment, and the gaps between the
    segments' images (where untranslated indices live) hold more than `slots` indices."""
    rows = 4 * slots + 64
    row0 = np.concatenate(([0], np.sort(rng.choice(np.arange(2, rows - 1), n - 1, replace=False)))).astype(np.int64)
    gaps = slots // n + 3 + rng.integers(0, 5, n)
    return row0, np.cumsum(gaps).astype(np.int64), rows


def translate(rows, row0, delta):
    rows = np.asarray(rows, dtype=np.int64)
    t = np.searchsorted(row0, rows, side="right") - 1
    return np.where(rows == INT_MAX, INT_MAX, rows + delta[np.clip(t, 0, len(delta) - 1)])


POOL = np.array([3.5, 1.0, 0.75, 0.5, 0.25, 0.0, -0.0, -0.25, -1.5, 1e-40, -3e38, -np.inf], dtype=np.float32)


def _scores(rng, order, n, lane_slots, k):
    if order == "plateau":
        return np.full(n, 0.625, np.float32)
    if order == "zeros":
        return rng.choice(np.array([0.0, -0.0], np.float32), n)
    if order == "reversed":
        return rng.choice(np.array([0.5, 0.25, -0.0], np.float32), n)
    pool = np.concatenate((POOL, rng.standard_normal(max(n // 4, 1)).astype(np.float32)))
    if order == "infs":
        pool = np.concatenate((pool, np.full(len(pool) // 3 + 1, np.inf, np.float32)))
    s = rng.choice(pool, n)
    if order == "lane" and len(lane_slots):  # the winners all sit in one lane's register slots
        top = 4.0 + np.sort(rng.choice(np.arange(1, 9, dtype=np.float32), len(lane_slots)))[::-1]
        s[lane_slots] = top
    return s


@functools.lru_cache(maxsize=None)
def build(c):
    rng = np.random.default_rng(_seed(c.name))
    src_id = np.concatenate([np.full(s.lists * s.len, j) for j, s in enumerate(c.srcs)])
    list_id = np.concatenate([np.repeat(np.arange(s.lists), s.len) for s in c.srcs])
    pos = np.concatenate([np.tile(np.arange(s.len), s.lists) for s in c.srcs])
    n_slots = len(src_id)
    mask = seg_mask(c)
    in_seg = np.array([(mask >> j) & 1 for j in src_id], dtype=bool)
    segments = None
    if c.seg_n:
        row0, delta, n_rows = _segments(rng, c.seg_n, n_slots)
        segments = (row0, delta)
        image = np.zeros(n_rows + int(delta[-1]) + 1, dtype=bool)
        image[translate(np.arange(n_rows), row0, delta)] = True
        free = np.flatnonzero(~image)  # dictionary indices no row translates to
        edge_rows = np.unique(np.concatenate((row0[1:] - 1, row0[1:])))
    layouts = []
    for s in c.srcs:
        if s.gather:  # finalize.hip's all-gather: rank after rank, each [m][len]
            row_stride, list_stride = s.len, c.m * s.len
            elems = s.lists * c.m * s.len
        else:
            list_stride = s.len + s.pad_list
            row_stride = s.lists * list_stride + s.pad_row
            elems = c.m * row_stride
        layouts.append(dict(scores=np.full(elems, np.inf, np.float32), idx=np.full(elems, 1, np.int32),
                            cnt=np.zeros((c.m, s.lists), np.int32) if s.counted else None, lists=s.lists, len=s.len,
                            row_stride=row_stride, list_stride=list_stride))
    last = n_slots - 1
    for mi in range(c.m):
        real = np.ones(n_slots, dtype=bool)
        holes = np.zeros(n_slots, dtype=bool)  # INT_MAX entries
        if c.real is None:
            for j, s in enumerate(c.srcs):
                if s.counted:
                    cnt = rng.integers(0, s.len + 1, s.lists)
                    cnt[rng.integers(0, s.lists)] = 0
                    cnt[rng.integers(0, s.lists)] = s.len
                    if j == len(c.srcs) - 1:
                        cnt[-1] = s.len
                    layouts[j]["cnt"][mi] = cnt
                    real[src_id == j] = (pos < cnt[list_id % s.lists])[src_id == j]
            holes = real & (rng.random(n_slots) < 0.1)
            holes[last] = False
        elif c.thin == "counts":
            # the counted sources' lists share what the uncounted sources leave of the target; the launch's last list
            # is served first (full whenever anything is left), then the others in random order: full, one partial, empty
            left = c.real - sum(s.lists * s.len for s in c.srcs if not s.counted)
            owners = [(j, l) for j, s in enumerate(c.srcs) if s.counted for l in range(s.lists)]
            for o in [len(owners) - 1] + list(rng.permutation(len(owners) - 1)):
                j, l = owners[o]
                layouts[j]["cnt"][mi, l] = min(c.srcs[j].len, left)
                left -= layouts[j]["cnt"][mi, l]
            assert left == 0
            for j, s in enumerate(c.srcs):
                if s.counted:
                    real[src_id == j] = (pos < layouts[j]["cnt"][mi][list_id % s.lists])[src_id == j]
        else:
            for j, s in enumerate(c.srcs):
                if s.counted:
                    layouts[j]["cnt"][mi] = s.len
            holes[rng.permutation(n_slots)[: n_slots - c.real]] = True
        live = real & ~holes
        n_live = int(live.sum())
        # distinct dictionary indices; the sources in seg_sources store the ROW that translates to theirs
        stored = np.zeros(n_slots, dtype=np.int64)
        if c.seg_n:
            n_seg = int((live & in_seg).sum())
            rows = edge_rows[: n_seg]
            if n_seg > len(rows):
                others = np.setdiff1d(np.arange(n_rows), rows)
                rows = np.concatenate((rows, rng.choice(others, n_seg - len(rows), replace=False)))
            stored[live & in_seg] = rng.permutation(rows)
            stored[live & ~in_seg] = rng.choice(free, int((live & ~in_seg).sum()), replace=False)
        else:
            stored[live] = rng.choice(4 * n_slots + 100, n_live, replace=False)
        if c.order == "reversed":  # indices fall where memory rises (rows among the sources that hold rows, indices among
            for group in (live & in_seg, live & ~in_seg):  # the others: a row is not an index, the two are never swapped)
                stored[group] = np.sort(stored[group])[::-1]
        lane_slots = np.flatnonzero(np.flatnonzero(live) % 64 == 37)[: c.k]
        sc = np.zeros(n_slots, dtype=np.float32)
        sc[live] = _scores(rng, c.order, n_live, lane_slots, c.k)
        if c.order in ("random", "lastslot") and live[last]:
            sc[last] = np.inf  # the winner sits in the last slot of the last list of the last source
        poison = np.where(np.arange(n_slots) % 2 == 0, np.float32(np.inf), np.float32(3e38))
        sc[~live] = poison[~live]
        stored[~real] = np.arange(n_slots)[~real] % 7
        stored[holes] = INT_MAX
        for j, lay in enumerate(layouts):
            sel = src_id == j
            e = mi * lay["row_stride"] + list_id[sel] * lay["list_stride"] + pos[sel]
            lay["scores"][e] = sc[sel]
            lay["idx"][e] = stored[sel]
    out_s = np.full((c.m, out_stride(c)), SENTINEL_S, np.float32)
    out_i = np.full((c.m, out_stride(c)), SENTINEL_I, np.int32)
    for lay in layouts:
        for a in lay.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return Built(tuple(layouts), segments, out_s, out_i)


def entries(c, b, mi, ignore_counts=False, no_segments=False, drop_last=False):
    """(scores, dictionary indices) of pattern mi's candidates in memory order; the keyword faults make a WRONG merge."""
    ss, ii = [], []
    for j, (s, lay) in enumerate(zip(c.srcs, b.sources)):
        l, p = np.divmod(np.arange(s.lists * s.len), s.len)
        e = mi * lay["row_stride"] + l * lay["list_stride"] + p
        keep = np.ones(len(e), dtype=bool)
        if lay["cnt"] is not None and not ignore_counts:
            keep &= p < lay["cnt"][mi][l]
        if drop_last and j == len(c.srcs) - 1:
            keep[-1] = False
        idx = lay["idx"][e].astype(np.int64)
        keep &= idx != INT_MAX
        if (seg_mask(c) >> j) & 1 and not no_segments:
            idx = translate(idx, *b.segments)
        ss.append(lay["scores"][e][keep])
        ii.append(idx[keep])
    return np.concatenate(ss), np.concatenate(ii)


def reference(c, b=None, memory_ties=False, **faults):
    """The expected output buffers (scores, idx), the caller's sentinel outside the merged columns included."""
    b = b or build(c)
    out_s, out_i = b.out_s.copy(), b.out_i.copy()
    for mi in range(c.m):
        s, i = entries(c, b, mi, **faults)
        s = s + np.float32(0)  # -0 -> +0
        with np.errstate(invalid="ignore"):
            order = np.argsort(-s, kind="stable") if memory_ties else np.lexsort((i, -s.astype(np.float64)))
        order = order[: c.k]
        row_s = np.full(c.k, -np.inf, np.float32)
        row_i = np.full(c.k, INT_MAX, np.int64)
        row_s[: len(order)] = s[order]
        row_i[: len(order)] = i[order]
        out_s[mi, c.out_offset:c.out_offset + c.k] = row_s
        out_i[mi, c.out_offset:c.out_offset + c.k] = row_i
    return out_s, out_i


def n_real(c, b, mi):
    return len(entries(c, b, mi)[0])


def counts_modes(c, plan):
    """How `plan` gets at the counts of the case's sources: in lanes (wave-per-pattern kernels, <= 64 lists), from memory
    per candidate, or none at all."""
    modes = set()
    for s in c.srcs:
        if s.counted:
            modes.add("lanes" if plan in CACHED and s.lists <= 64 else "memory")
    return modes or {"none"}


def cells(c):
    """The forks the case reaches when every kernel that holds it is forced: (plan, counts mode, sources, segments,
    packed).  packed: the wave-per-pattern kernels' LDS packing - True / False per pattern; None for the other kernels."""
    b = build(c)
    reals = [n_real(c, b, mi) for mi in range(c.m)]
    out = set()
    for p in plans_for(c):
        packs = {r <= packed_capacity(p) for r in reals} if p in CACHED else {None}
        for mode in counts_modes(c, p):
            for pk in packs:
                out.add((PLANS[p], mode, len(c.srcs), bool(c.seg_n), pk))
    return out


def _cases():
    out = []
    # ---- the grid: sources x segments x counts mode x (few candidates | more than 512 real ones) ---------------------
    for n_src in (1, 2, 3):
        for seg_n in (0, 2):
            for mode in ("none", "lanes", "memory"):
                for size in ("small", "wide"):
                    k = 20
                    if size == "small":
                        chunk = {"none": Src(6, 8), "lanes": Src(64, 1, True), "memory": Src(65, 1, True)}[mode]
                    else:  # up to 768 candidates, more than 512 of them real: <12> runs its rounds over the registers
                        chunk = {"none": Src(20, 32), "lanes": Src(32, 20, True), "memory": Src(80, 8, True)}[mode]
                    third = Src(3 if size == "small" else 5, 20)
                    srcs = {1: (chunk,), 2: (Src(1, k), chunk), 3: (Src(1, k), third, chunk)}[n_src]
                    mask = 0 if not seg_n else (1 if n_src == 1 else (~0 << 1) & ((1 << n_src) - 1))
                    real = sum(s.lists * s.len for s in srcs) - 60 if size == "wide" and mode != "none" else None
                    out.append(Case(f"grid-{n_src}src-seg{seg_n}-{mode}-{size}", 5, k, srcs, seg_n=seg_n, seg_sources=mask,
                                    real=real))
    # ---- candidate totals either side of every plan boundary (len in {1, 8, 20, 32} + a running list of len k) --------
    for total in (256, 257, 768, 769, 1536, 1537, 3072, 3073, 6144, 6145, 16384, 16385, 20001):
        k = 20
        rest = total - k
        n32 = rest // 32
        srcs = [Src(1, k)]
        if n32:
            srcs.append(Src(n32, 32, counted=total % 2 == 0))
        if rest - 32 * n32:
            srcs.append(Src(rest - 32 * n32, 1))
        assert sum(s.lists * s.len for s in srcs) == total
        out.append(Case(f"total-{total}", 3 if total < 4000 else 2, k, tuple(srcs)))
    for total, ln in ((768, 8), (769, 1), (1536, 20), (3072, 32)):  # one source, other list lengths
        lists = total // ln
        out.append(Case(f"total1-{lists}x{ln}", 3, 20, (Src(lists, ln, counted=True),), seg_n=1, seg_sources=1))
    # ---- real candidates around the packing limit of every NK ---------------------------------------------------------
    for name, srcs, limit in (("nk4", (Src(1, 32, True), Src(7, 32, True)), 256),
                              ("nk12", (Src(1, 20, True), Src(37, 20, True), Src(8, 1, True)), 512)):
        total = sum(s.lists * s.len for s in srcs)
        for real in sorted({0, 1, limit - 1, limit, min(limit + 1, total), total}):
            for thin in ("counts", "intmax"):
                out.append(Case(f"real-{name}-{real}-{thin}", 3, 20, srcs, real=real, thin=thin,
                                order="plain" if real < total else "random"))
    for real in (511, 512, 513):  # the same limit from the larger wave kernels' own candidate ranges
        out.append(Case(f"real-nk24-{real}", 2, 20, (Src(40, 32, True),), real=real, thin="counts", order="plain"))
        out.append(Case(f"real-nk48-{real}", 2, 32, (Src(1, 32, True), Src(65, 32, True)), real=real, thin="counts", order="plain"))
    # ---- k and output placement ---------------------------------------------------------------------------------------
    chunk = Src(12, 20, counted=True)
    for k in (1, 20, 32, 33, 70):
        out.append(Case(f"k{k}", 3, k, (Src(1, k), chunk)))
    out.append(Case("k70-pads", 3, 70, (Src(3, 8, True),)))  # more ranks than candidates
    out.append(Case("pass-offset32-k38", 5, 38, (Src(9, 32, True),), out_stride=70, out_offset=32))  # local_pass
    out.append(Case("pass-offset32-k20", 5, 20, (Src(9, 20, True),), out_stride=70, out_offset=32))
    out.append(Case("pass-offset0-k32", 5, 32, (Src(9, 32, True),), out_stride=70, out_offset=0))
    # ---- m: the last workgroup of the wave-per-pattern kernels is partial ----------------------------------------------
    for m in (1, 3, 5, 9):
        out.append(Case(f"m{m}", m, 20, (Src(1, 20), Src(16, 20, True), Src(2, 20)), seg_n=2, seg_sources=6))
    # ---- counts: a counted source in each position, all counted, 64 against 65 lists -----------------------------------
    for at in range(3):
        srcs = tuple(Src(5 + j, (8, 20, 32)[j], counted=j == at) for j in range(3))
        out.append(Case(f"counted-at{at}", 5, 20, srcs))
    out.append(Case("counted-all", 5, 20, (Src(64, 1, True), Src(65, 1, True), Src(7, 20, True))))
    out.append(Case("counted-64-lists", 5, 20, (Src(1, 20), Src(64, 8, True))))
    out.append(Case("counted-65-lists", 5, 20, (Src(1, 20), Src(65, 8, True))))
    # ---- layouts ----------------------------------------------------------------------------------------------------
    out.append(Case("padded", 5, 20, (Src(1, 20, pad_row=12), Src(9, 20, True, pad_list=4, pad_row=7), Src(3, 8, pad_list=1))))
    out.append(Case("padded-seg", 3, 33, (Src(11, 32, True, pad_list=32, pad_row=1),), seg_n=16, seg_sources=1))
    for ranks in (2, 8):
        out.append(Case(f"gather-{ranks}", 5, 70, (Src(ranks, 70, gather=True),)))
    # ---- segments -----------------------------------------------------------------------------------------------------
    for seg_n in (1, 2, 16):
        out.append(Case(f"seg{seg_n}-later", 5, 20, (Src(1, 20), Src(12, 20, True), Src(4, 20)), seg_n=seg_n, seg_sources=6))
        out.append(Case(f"seg{seg_n}-only", 5, 20, (Src(20, 8),), seg_n=seg_n, seg_sources=1))
    out.append(Case("seg16-k70", 3, 70, (Src(1, 70), Src(1, 70)), seg_n=16, seg_sources=2))  # keep_n > 32: two full lists
    # ---- order --------------------------------------------------------------------------------------------------------
    for order in ("reversed", "plateau", "zeros", "infs", "lastslot", "lane"):
        out.append(Case(f"order-{order}", 5, 20, (Src(1, 20), Src(30, 20, True), Src(6, 8)), order=order))
        out.append(Case(f"order-{order}-seg", 3, 33, (Src(1, 33), Src(70, 32)), seg_n=2, seg_sources=2, order=order))
    out.append(Case("order-lane-one-source", 3, 20, (Src(48, 32),), order="lane"))  # 24 slots per lane: 20 winners in lane 37
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_id(c):
    return c.name


# ---- the float64 merge (merge64_kernel) --------------------------------------------------------------------------------
Case64 = namedtuple("Case64", "name m k lists len run in_place pad cert", defaults=(True, True, 0, None))
SENTINEL64_S, SENTINEL64_I = 7.25, -7


@functools.lru_cache(maxsize=None)
def build64(c):
    """Running list (or None), candidate buffers and, for the certification cases, cand_s32 and what each pattern's entry
    of rank k - 1 is set to.  Scores repeat, indices repeat, identical pairs occur; NaN scores and INT_MAX indices are
    empty entries."""
    rng = np.random.default_rng(_seed(c.name.split("/")[0]))
    list_stride = c.len + c.pad
    row_stride = c.lists * list_stride + c.pad
    cs = np.full(c.m * row_stride, np.inf)
    ci = np.full(c.m * row_stride, 1, np.int32)
    pool = np.concatenate(([0.0, -0.0, 0.5, 0.5, -1.0, 2.0**-30], np.round(rng.standard_normal(8) * 64) / 64))  # (all float32 values)
    run = None
    if c.run:
        rs = np.sort(rng.choice(pool, (c.m, c.k)), axis=1)[:, ::-1].copy()
        ri = rng.integers(0, 50, (c.m, c.k)).astype(np.int32)
        rs[:, c.k - c.k // 4:] = -np.inf  # a running list that is not full yet
        ri[:, c.k - c.k // 4:] = INT_MAX
        run = (rs, ri)
    for mi in range(c.m):
        l, p = np.divmod(np.arange(c.lists * c.len), c.len)
        e = mi * row_stride + l * list_stride + p
        s = rng.choice(pool, len(e))
        i = rng.integers(0, 50, len(e)).astype(np.int32)
        s[rng.random(len(e)) < 0.1] = np.nan
        i[rng.random(len(e)) < 0.1] = INT_MAX
        cs[e], ci[e] = s, i
    return run, cs, ci, row_stride, list_stride


def entries64(c, mi):
    run, cs, ci, row_stride, list_stride = build64(c)
    l, p = np.divmod(np.arange(c.lists * c.len), c.len)
    e = mi * row_stride + l * list_stride + p
    s, i = cs[e], ci[e].astype(np.int64)
    if run is not None:
        s, i = np.concatenate((run[0][mi], s)), np.concatenate((run[1][mi].astype(np.int64), i))
    empty = np.isnan(s) | (i == INT_MAX)
    return np.where(empty, -np.inf, s), np.where(empty, INT_MAX, i)


def reference64(c):
    """(scores, idx, uncertified): order (score descending, index ascending, position ascending), identical pairs both
    kept.  With fewer than k entries in all (only possible without a running list) the ranks behind them are NOT written
    - they keep the caller's content - and no entry holds rank k - 1, so the pattern is never counted as uncertified:
    what the kernel does, and harmless, since the sweep always passes a running list.  No case holds a score of -inf
    with a valid index: the kernel uses -inf as its mark of an empty entry and would return INT_MAX for it, and a
    rescored score is a correlation, never -inf."""
    out_s = np.full((c.m, c.k), SENTINEL64_S)
    out_i = np.full((c.m, c.k), SENTINEL64_I, np.int64)
    uncertified = 0
    for mi in range(c.m):
        s, i = entries64(c, mi)
        order = np.lexsort((np.arange(len(s)), i, -s))[: c.k]
        out_s[mi, : len(order)] = s[order]
        out_i[mi, : len(order)] = i[order]
        if c.cert is not None and len(order) == c.k:
            last32 = np.float32(c.cert["last32"][mi])
            eps = max(np.float32(8) * np.float32(c.cert["max_diff"]), np.float32(c.cert["eps_floor"]))
            ok = c.cert["enumerated_all"] or last32 == -np.inf or s[order[-1]] > float(last32) + float(eps)
            uncertified += not ok
    return out_s, out_i, (uncertified if c.cert is not None else None)


def cert_inputs(c):
    """cand_s32 (m, 3) with the screened-last score in column 1."""
    s32 = np.full((c.m, 3), np.inf, np.float32)
    s32[:, 1] = c.cert["last32"]
    return dict(cand_s32=s32, s32_col=1, max_diff=c.cert["max_diff"], eps_floor=c.cert["eps_floor"],
                enumerated_all=c.cert["enumerated_all"])


def _kth(c):
    return np.array([np.sort(entries64(c, mi)[0])[::-1][c.k - 1] for mi in range(c.m)])


def _cases64():
    out = [Case64("plain", 5, 20, 3, 8), Case64("separate", 5, 20, 3, 8, in_place=False),
           Case64("no-run", 5, 20, 4, 8, run=False, in_place=False), Case64("padded", 3, 7, 5, 3, in_place=False, pad=2),
           Case64("k1", 3, 1, 1, 5), Case64("k70", 2, 70, 1, 32),
           Case64("fewer-than-k", 3, 20, 2, 8, run=False, in_place=False),
           Case64("lds-64k", 2, 20, 1, 5441), Case64("lds-over-64k", 2, 20, 1, 5442),
           Case64("lds-150k", 1, 20, 1, 12780)]
    # certification: sc > last32 + max(8 max_diff, eps_floor), every value a short binary fraction.  The k-th best score
    # of a pattern is whatever the seeded data gives; last32 is placed against it: at the boundary (fails: not above),
    # one float32 step below (passes), far above (fails), -inf (passes).
    base = Case64("cert", 8, 20, 3, 8)
    kth = _kth(base)
    for tag, max_diff, floor in (("diff", 2.0**-10, 2.0**-8), ("floor", 2.0**-12, 2.0**-8)):
        eps = max(8 * max_diff, floor)
        assert eps == 2.0**-7 if tag == "diff" else eps == 2.0**-8
        # (the pool's scores are multiples of 2^-6, so `kth - eps` is exact in float32)
        last = np.empty(8, np.float32)
        for mi in range(8):
            at = np.float32(kth[mi]) - np.float32(eps)
            last[mi] = (at, np.nextafter(at, np.float32(-np.inf)), at + np.float32(1), -np.inf)[mi % 4]
        for every in (False, True):
            out.append(base._replace(name=f"cert/{tag}{'-enumerated-all' if every else ''}",
                                     cert=_freeze(last32=last, max_diff=max_diff, eps_floor=floor, enumerated_all=every)))
    return out


class _Frozen(dict):
    def __hash__(self):
        return hash((tuple(np.asarray(self["last32"]).tolist()), self["max_diff"], self["eps_floor"], self["enumerated_all"]))


def _freeze(**kw):
    return _Frozen(kw)


CASES64 = _cases64()
LDS_REFUSED = Case64("lds-refused", 1, 20, 1, 12781)  # (20 + 12 781) x 12 bytes > 150 KB: an error, nothing launched


# ---- fill_segments_kernel ---------------------------------------------------------------------------------------------
GUARD = 0xDEADBEEF
THRESHOLD_NONE = 0x007FFFFF
FILL_LAUNCHES = {
    # name: ranges of (byte offset, words, value, bound_used); the buffer starts on a 256-byte boundary
    "aligned": [(64, 64, 0x11111111, -1)],
    "unaligned-start": [(68, 64, 0x22222222, -1)],
    "aligned-odd-words": [(64, 63, 0x33333333, -1), (512, 5, 0x44444444, -1), (640, 1, 0x55555555, -1)],
    "empty-range": [(64, 0, 0x66666666, -1), (128, 8, 0x77777777, -1)],
    "all-empty": [(64, 0, 1, -1), (128, 0, 2, 0)],
    "bound": [(64, 96, 9, 0), (1024, 96, 9, 1), (2048, 100, 9, 31), (3072, 64, 9, 32), (4100, 37, 9, 5)],
    # eight ranges of unequal length in one launch, constants and bound patterns, starts at every remainder modulo 16 bytes
    "eight": [(64 + 20480 * i + 4 * (i % 4), (3, 250, 0, 17, 4096, 64, 1, 1300)[i], 0x100 + i, -1 if i % 2 == 0 else 7)
              for i in range(8)],
    "long": [(256, 300000, 0xABCDEF01, -1), (256 + 4 * 300004, 300001, 0xABCDEF02, -1), (256 + 4 * 600016, 270001, 3, 12)],
}


def fill_buffer(ranges):
    end = max(off // 4 + n for off, n, _, _ in ranges) + 16
    return np.full(end, GUARD, np.uint32)


def fill_reference(ranges):
    buf = fill_buffer(ranges)
    for off, n, value, used in ranges:
        i = np.arange(n)
        buf[off // 4: off // 4 + n] = value if used < 0 else np.where(i % 32 < used, THRESHOLD_NONE, 0xFFFFFFFF)
    return buf
