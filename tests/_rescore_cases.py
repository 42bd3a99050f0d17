"""Case table and two references for rescore_kernel on its own (csrc/rescore.hip, through kpdi_rescore_selftest): seeded,
pure NumPy, no GPU.  tests/test_host_rescore_cases.py checks the table (the kernel model agrees with the precise
reference, every named wrong variant of the model fails some case, every dtype pair / reduction length / window edge is
reached), tests/test_gpu_rescore.py runs it through the kernel.

The kernel's contract, as `reference` states it.  Per pattern m and column j of [cand_offset, cand_offset + n_cand):
the candidate index cand_i[m][j] is global; INT_MAX or an index outside [global_start, global_start + n_chunk) scores
-inf; otherwise the score is the reference's formula (cast, centring under `ncc`, L2 normalisation, dot product) over the
k kept pixels (pix_map, or the first k of npix) of experimental row row_map[m] (or m) and dictionary row index -
global_start, to 1e-12 - evaluated here in np.longdouble - unless either pattern is DEGENERATE by include/kpdi.h
("Degenerate patterns"), a verdict taken on the FLOAT32 CAST of its kept pixels whatever the dtype and the arithmetic:
then it is exactly +0.0.  Columns outside the window keep what the caller put there (FILL: a NaN with a payload, compared
bit for bit).  max_diff ends at max(what it started from, float32(|score - cand_s|) over the entries that were scored).

cand_s is float32(precise score) plus an offset of at most 1e-6, and every case plants ONE offset of 3e-4 on a scored
entry: the expected max_diff is then known to 2 float32 ulps (the kernel's double difference is off by at most the score
tolerance 1e-12, below one ulp at 3e-4 = 2.9e-11, then rounded once), and a max_diff that missed a wave or a workgroup
comes back near 1e-6 instead."""
import functools
import math
from collections import namedtuple

import numpy as np

INT_MAX = 2**31 - 1
NCC, NDP = 0, 1
TOL = 1e-12  # the float64 path's contract: tests/test_gpu_f64.py TOL, the header of csrc/rescore.hip
FILL = np.array([0x7FF80000DEADBEEF], dtype=np.uint64).view(np.float64)[0]
FILL_BITS = 0x7FF80000DEADBEEF
PLANT = 3e-4
DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.float16, np.float32, np.int32, np.uint32, np.float64)
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 3600)
N_CANDS = (1, 2, 3, 4, 5, 33)
LONG = np.finfo(np.longdouble).eps < 1e-18
OUTSIDE, SKIPPED, DEGENERATE, ORDINARY = 0, 1, 2, 3

# exp / dic: a dtype (random data over the type's whole range) or a list of row recipes (_row); pix: None | "perm" (a
# permutation of a strict subset of npix) | "outlier" (the same, pix_map[0] at a 1e6 pixel); rows: None | "reversed" | a
# list; cands: "random" | "edges" | "all" (every dictionary row once); plant: (row, column) of the 3e-4 offset, "skipped"
# (a second one, on an entry that is not scored) or None = drawn; init: "below" | "equal" | "above" the expected max_diff
Case = namedtuple("Case", "name group metric exp dic m_all m n_chunk npix k pix rows global_start cand_offset n_cand pad "
                          "cands plant init deg_exp deg_dic",
                  defaults=(None, None, 0, 0, None, 3, "random", None, "below", None, None))
Built = namedtuple("Built", "case exp dic row_map pix_map k cand_s cand_i fill init want kind want_md planted")


def case_id(c):
    return c.name


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2**32)


# ---- data ---------------------------------------------------------------------------------------------------------------
def _random(rng, dtype, shape):
    """The whole range of the type: negative values for the signed integers, values >= 2^31 for uint32, subnormals and
    values near 65504 for float16 (a signedness or width slip moves a score by far more than the tolerance)."""
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)
    if dt == np.float16:
        a = rng.uniform(-1.0, 1.0, shape)
        pick = rng.random(shape)
        a = np.where(pick < 0.15, rng.uniform(-6e-5, 6e-5, shape), a)
        a = np.where(pick > 0.85, rng.uniform(60000.0, 65504.0, shape) * rng.choice([-1.0, 1.0], shape), a)
        return a.astype(np.float16)
    return rng.random(shape).astype(dt)


def _row(rng, recipe, npix, dtype, kept):
    """One pattern from a recipe: ("random",) | ("const", v) | ("poke", v, value, inside) - constant v with ONE pixel
    set to `value`, inside the kept area or outside it | ("rpoke", value, inside) - the same on random data |
    ("scaled", a, b) - a + b * u, u random in [0, 1)."""
    kind = recipe[0]
    inside = np.zeros(npix, bool)
    inside[kept] = True
    if kind == "random":
        return _random(rng, dtype, npix)
    if kind == "const":
        return np.full(npix, recipe[1], dtype)
    if kind in ("poke", "rpoke"):
        row = np.full(npix, recipe[1], dtype) if kind == "poke" else _random(rng, dtype, npix)
        where = np.flatnonzero(inside if recipe[-1] else ~inside)
        row[where[len(where) // 2]] = recipe[-2]
        return row
    if kind == "scaled":
        return (recipe[1] + recipe[2] * rng.random(npix)).astype(dtype)
    raise ValueError(kind)


def _patterns(rng, spec, rows, npix, kept):
    if isinstance(spec, tuple):  # (dtype, recipes)
        dtype, recipes = spec
        assert len(recipes) == rows
        return np.stack([_row(rng, r, npix, dtype, kept) for r in recipes])
    return _random(rng, spec, (rows, npix))


def dtype_of(spec):
    return np.dtype(spec[0] if isinstance(spec, tuple) else spec)


# ---- the precise reference ----------------------------------------------------------------------------------------------
def _hp(a):
    return np.asarray(a).astype(np.longdouble if LONG else np.float64)


def _sum(a):
    """Sums along the last axis: np.longdouble where it has a 64-bit mantissa, else exactly rounded (math.fsum)."""
    if LONG:
        return a.sum(axis=-1)
    flat = a.reshape(-1, a.shape[-1])
    return np.array([math.fsum(r.tolist()) for r in flat]).reshape(a.shape[:-1])


def degenerate32(kept, metric):
    """include/kpdi.h "Degenerate patterns" on the float32 cast of the kept pixels: NaN or inf among them; `ncc` - all
    equal; either metric - a float32 sum of (centred) squares that is not positive and finite."""
    with np.errstate(all="ignore"):
        f = np.asarray(kept).astype(np.float32)
        if not np.isfinite(f).all():
            return True
        if metric == NCC:
            if f.min() == f.max():
                return True
            f = f - np.float32(f.astype(np.float64).mean())
        total = np.float32((f * f).astype(np.float64).sum())
        return not (total > 0 and total < np.inf)


def precise_scores(x, ys, metric):
    """The reference's formula for one experimental pattern (k,) against patterns (n, k), no degeneracy rule."""
    x, ys = _hp(x), _hp(ys)
    if metric == NCC:
        x = x - _sum(x) / x.size
        ys = ys - (_sum(ys) / x.size)[:, None]
    return _sum(x * ys) / (np.sqrt(_sum(x * x)) * np.sqrt(_sum(ys * ys)))


def _layout(c, rng):
    npix, k = c.npix, c.k
    pix_map = None
    if c.pix:
        pix_map = rng.permutation(np.arange(1, npix))[:k].astype(np.int32)  # pixel 0 is never kept
        assert k < npix - 1
        if k > 1 and not (np.diff(pix_map) < 0).any():
            pix_map = pix_map[::-1].copy()  # never monotone
    kept = np.arange(k) if pix_map is None else pix_map
    row_map = None
    if c.rows == "reversed":
        row_map = np.arange(c.m_all - 1, -1, -1, dtype=np.int32)
    elif c.rows is not None:
        row_map = np.array(c.rows, dtype=np.int32)
    return pix_map, kept, row_map


def _candidates(c, rng):
    gs, n, m, nc = c.global_start, c.n_chunk, c.m, c.n_cand
    if c.cands == "all":
        assert nc == n
        return np.tile(np.arange(gs, gs + n), (m, 1))
    ci = rng.integers(gs, gs + n, (m, nc))
    if c.cands == "edges":
        special = [gs - 1, gs, gs + n - 1, gs + n, INT_MAX]  # every one of them in every case
        for t in range(m * nc):
            if nc == 1 or t % 2 == 0:
                ci[t // nc, t % nc] = special[(t if nc == 1 else t // 2) % 5]
        if nc >= 3:
            ci[0, 1] = INT_MAX              # in the middle of a list
        if nc >= 2:
            ci[1::2, nc - 1] = ci[1::2, 0]  # duplicates within a list
    return ci


@functools.lru_cache(maxsize=None)
def build(name):
    c = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    pix_map, kept, row_map = _layout(c, rng)
    exp = _patterns(rng, c.exp, c.m_all, c.npix, kept)
    dic = _patterns(rng, c.dic, c.n_chunk, c.npix, kept)
    if c.pix == "outlier":  # the kernel shifts a dictionary row by its first kept pixel: make that one the brightest,
        exp[:, kept[0]] = 1e6  # and put something larger still where a shift by pixel 0 would look
        dic[:, kept[0]] = 1e6
        dic[:, 0] = 1e9
    stride = c.cand_offset + c.n_cand + c.pad
    cols = slice(c.cand_offset, c.cand_offset + c.n_cand)
    # outside the window: valid indices and float32 scores nobody may read, the payload NaN nobody may overwrite
    cand_i = np.full((c.m, stride), c.global_start, dtype=np.int32)
    cand_s = np.full((c.m, stride), 9.0, dtype=np.float32)
    cand_i[:, cols] = _candidates(c, rng)
    want = np.full((c.m, stride), FILL)
    kind = np.zeros((c.m, stride), dtype=np.int8)
    deg_d = np.array([degenerate32(dic[r, kept], c.metric) for r in range(c.n_chunk)])
    for mi in range(c.m):
        row = mi if row_map is None else row_map[mi]
        local = cand_i[mi, cols].astype(np.int64) - c.global_start
        ok = (cand_i[mi, cols] != INT_MAX) & (local >= 0) & (local < c.n_chunk)
        deg_e = degenerate32(exp[row, kept], c.metric)
        w, kd = np.full(c.n_cand, -np.inf), np.full(c.n_cand, SKIPPED, dtype=np.int8)
        if ok.any():
            loc = local[ok]
            deg = deg_e | deg_d[loc]
            with np.errstate(all="ignore"):
                s = precise_scores(exp[row, kept], dic[loc][:, kept], c.metric).astype(np.float64)
            w[ok] = np.where(deg, 0.0, s)
            kd[ok] = np.where(deg, DEGENERATE, ORDINARY)
        want[mi, cols], kind[mi, cols] = w, kd
    # the float32 screen's scores: the precise ones rounded, off by up to 1e-6, one of them by 3e-4
    scored = np.argwhere(kind >= DEGENERATE)
    offs = rng.uniform(-1e-6, 1e-6, (c.m, stride))
    planted = None
    if len(scored):
        planted = tuple(scored[rng.integers(len(scored))]) if c.plant in (None, "skipped") else (c.plant[0], c.cand_offset + c.plant[1])
        assert kind[planted] >= DEGENERATE, (name, planted)
        offs[planted] = PLANT
    sc = kind >= DEGENERATE
    cand_s[sc] = (want[sc].astype(np.float32).astype(np.float64) + offs[sc]).astype(np.float32)
    cand_s[kind == SKIPPED] = rng.uniform(-1, 1, int((kind == SKIPPED).sum())).astype(np.float32)
    if c.plant == "skipped":
        skipped = np.argwhere(kind == SKIPPED)
        cand_s[tuple(skipped[0])] = np.float32(0.5)
    diffs = np.abs(want[sc] - cand_s[sc].astype(np.float64)).astype(np.float32)
    top = diffs.max() if diffs.size else np.float32(0)
    init = {"below": np.float32(1e-5), "equal": top, "above": np.float32(1e-2), "zero": np.float32(0)}[c.init]
    return Built(c, exp, dic, row_map, pix_map, c.k, cand_s, cand_i, np.full((c.m, stride), FILL), init, want, kind,
                 max(init, top), planted)


def check(b, got, got_md):
    """What tests/test_gpu_rescore.py asserts of the kernel (and the host test of the model): a list of complaints, and
    the largest |score - reference| over the ordinary entries."""
    bad = []
    bits = np.ascontiguousarray(got).view(np.uint64)
    for what, sel, want_bits in (("outside the window", b.kind == OUTSIDE, FILL_BITS),
                                 ("skipped", b.kind == SKIPPED, 0xFFF0000000000000),
                                 ("degenerate", b.kind == DEGENERATE, 0)):
        wrong = np.argwhere(sel & (bits != np.uint64(want_bits)))
        if len(wrong):
            bad.append(f"{what}: {len(wrong)} entries, first {wrong[0].tolist()} = {got[tuple(wrong[0])]!r}")
    o = b.kind == ORDINARY
    err = np.abs(got[o] - b.want[o])
    worst = float(np.nanmax(err)) if err.size and not np.isnan(err).all() else 0.0
    if not (err <= TOL).all():
        at = np.argwhere(o)[np.flatnonzero(~(err <= TOL))[0]]
        bad.append(f"scores: {int((~(err <= TOL)).sum())} beyond {TOL}, worst {worst:.3e}, first {at.tolist()} = "
                   f"{got[tuple(at)]!r}, want {b.want[tuple(at)]!r}")
    if np.isnan(got[b.kind != OUTSIDE]).any():
        bad.append("NaN inside the window")
    gm, wm = np.float32(got_md), np.float32(b.want_md)
    ulps = abs(int(gm.view(np.uint32)) - int(wm.view(np.uint32)))
    allowed = 0 if b.init == b.want_md and b.case.init != "equal" else 2  # nothing reached it: it comes back as it went
    if not (gm >= 0 and ulps <= allowed):
        bad.append(f"max_diff {gm!r}, want {wm!r} within {allowed} ulps (started from {b.init!r})")
    return bad, worst


# ---- the kernel model ---------------------------------------------------------------------------------------------------
FAULTS = (
    "I8 read as U8", "U32 read as I32", "F16 read as 2-byte integers", "pix_map ignored",
    "pix_map[0] not used for the shift", "row_map ignored", "mean over npix instead of k",
    "the elements beyond the last multiple of 64 dropped", "ndp centred", "the window test local <= n_chunk",
    "global_start ignored", "cand_offset ignored", "only n_cand - n_cand % 4 candidates scored", "max_diff from wave 0 only",
    "max_diff from the last workgroup only", "max_diff including the -inf entries", "max_diff overwritten instead of maxed",
    "a constant pattern scored NaN", "degeneracy decided on the doubles",
)


def _raw(a, fault):
    if fault == "I8 read as U8" and a.dtype == np.int8:
        a = a.view(np.uint8)
    if fault == "U32 read as I32" and a.dtype == np.uint32:
        a = a.view(np.int32)
    if fault == "F16 read as 2-byte integers" and a.dtype == np.float16:
        a = a.view(np.int16)
    return a.astype(np.float64)


def _f32_degenerate(lo, hi, mean, norm2, ncc, fault):
    """rescore.hip's f32_degenerate: the float32 screen's verdict from the extremes, the mean and the sum of squares."""
    with np.errstate(all="ignore"):
        if fault == "degeneracy decided on the doubles":  # what the kernel did before it followed the float32 cast
            return bool((ncc and lo == hi) or not 0 < norm2 < np.inf)
        lo, hi, mf = np.float32(lo), np.float32(hi), np.float32(mean)
        vmax = np.fmax(hi - mf, mf - lo)
        return bool((ncc and lo == hi) or not 0 < vmax * vmax < np.inf or not 0 < np.float32(norm2) < np.inf)


def model(b, fault=None):
    """rescore_kernel in plain float64 NumPy: the same formulas (one-pass variance of a dictionary row shifted by its
    first kept pixel, the dot product corrected by the residual sum of the centred experimental pixels), NumPy's
    summation order.  `fault`: one of FAULTS, a kernel that is wrong in that way.  Returns (cand_s64, max_diff)."""
    c = b.case
    out = b.fill.copy()
    centre = c.metric != NDP or fault == "ndp centred"
    k = b.k
    pm = np.arange(k) if b.pix_map is None or fault == "pix_map ignored" else b.pix_map[:k]
    off = 0 if fault == "cand_offset ignored" else c.cand_offset
    n_cand = c.n_cand - c.n_cand % 4 if fault == "only n_cand - n_cand % 4 candidates scored" else c.n_cand
    gs = 0 if fault == "global_start ignored" else c.global_start
    worst = np.zeros((c.m, 4), dtype=np.float32)
    edge = c.n_chunk + 1 if fault == "the window test local <= n_chunk" else c.n_chunk
    with np.errstate(all="ignore"):
        for mi in range(c.m):
            row = mi if b.row_map is None or fault == "row_map ignored" else b.row_map[mi]
            x = _raw(b.exp[row], fault)[pm]
            mx = x.sum() / (c.npix if fault == "mean over npix instead of k" else k) if centre else 0.0
            v = x - mx
            sxx, sx_res = (v * v).sum(), v.sum()
            x_deg = _f32_degenerate(np.fmin.reduce(x), np.fmax.reduce(x), mx, sxx, centre, fault)
            for j in range(n_cand):
                idx, s32 = int(b.cand_i[mi, off + j]), b.cand_s[mi, off + j]
                local = idx - gs
                score = -np.inf
                if idx != INT_MAX and 0 <= local < edge:
                    yrow = _raw(b.dic[local % c.n_chunk], fault)  # (% n_chunk: the faulty window reads SOME row)
                    yraw = yrow[pm]
                    y0 = (yrow[0] if fault == "pix_map[0] not used for the shift" else yraw[0]) if centre else 0.0
                    y, xs = yraw - y0, v
                    if fault == "the elements beyond the last multiple of 64 dropped":
                        y, xs = y[: k - k % 64], v[: k - k % 64]
                    s1, s2, sxy = y.sum(), (y * y).sum(), (xs * y).sum()
                    syy = s2 - s1 * s1 / k if centre else s2
                    if centre:
                        sxy -= (s1 / k) * sx_res
                    deg = x_deg or _f32_degenerate(np.fmin.reduce(yraw), np.fmax.reduce(yraw), y0 + s1 / k if centre else 0.0, syy, centre,
                                                    fault)
                    score = (np.nan if fault == "a constant pattern scored NaN" else 0.0) if deg else sxy / (np.sqrt(sxx) * np.sqrt(syy))
                    if score != score and fault != "a constant pattern scored NaN":
                        score = 0.0
                if score > -np.inf or fault == "max_diff including the -inf entries":
                    worst[mi, j % 4] = np.fmax(worst[mi, j % 4], np.abs(np.float32(score - np.float64(s32))))
                out[mi, off + j] = score
    if fault == "max_diff from wave 0 only":
        worst = worst[:, :1]
    if fault == "max_diff from the last workgroup only":
        worst = worst[-1:]
    w = worst.max()
    if fault == "max_diff overwritten instead of maxed":
        return out, (w if w > 0 else b.init)
    return out, max(b.init, w)


# ---- the table ----------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    names = {NCC: "ncc", NDP: "ndp"}
    # every pair of dtypes, both metrics: 5 patterns against 9 of 12 x 11 pixels, all kept
    for metric in (NCC, NDP):
        for e in DTYPES:
            for d in DTYPES:
                out.append(Case(f"dtypes-{np.dtype(e).name}-{np.dtype(d).name}-{names[metric]}", "dtypes", metric, e, d, 5, 5, 9,
                                132, 132, n_cand=6))
    # reduction lengths: 256 per stride for the experimental statistics, 64 per stride for a candidate
    for k in LENGTHS:
        metric = NDP if k == 1 else NCC
        big = k == 3600
        m, n = (3, 6) if big else (4, 11)
        out.append(Case(f"length-{k}", "lengths", metric, np.float32, np.float32, m, m, n, k + (0 if big else 3), k, n_cand=5))
        npix = 61 * 61 if big else k + 29
        out.append(Case(f"length-{k}-mapped", "lengths", metric, np.uint16 if k % 2 and k != 65 else np.float32, np.float32, m, m, n, npix,
                        k, pix="outlier" if k == 65 else "perm", n_cand=5))
    out.append(Case("length-257-ndp-mapped", "lengths", NDP, np.int16, np.float64, 4, 4, 11, 300, 257, pix="perm", n_cand=5))
    # rows
    out.append(Case("rows-reversed", "rows", NCC, np.uint8, np.float32, 6, 6, 9, 100, 100, rows="reversed", n_cand=7))
    out.append(Case("rows-3-of-17", "rows", NCC, np.uint8, np.float32, 17, 3, 9, 100, 90, pix="perm", rows=[16, 4, 9], n_cand=7))
    # the candidate window
    for gs in (0, 1000):
        for off in (0, 5):
            for nc in N_CANDS:
                out.append(Case(f"window-start{gs}-offset{off}-cand{nc}", "window", NCC, np.uint8, np.float32, 5, 5, 7, 80, 80,
                                global_start=gs, cand_offset=off, n_cand=nc, cands="edges"))
    # max_diff: the planted entry in every wave (column % 4) of the first, a middle and the last workgroup
    for wg, mi in (("first", 0), ("middle", 2), ("last", 4)):
        for wave in range(4):
            out.append(Case(f"maxdiff-{wg}-wave{wave}", "maxdiff", NCC, np.uint8, np.float32, 5, 5, 12, 80, 80, n_cand=9,
                            plant=(mi, 4 + wave)))
    for init in ("zero", "equal", "above"):
        out.append(Case(f"maxdiff-init-{init}", "maxdiff", NCC, np.uint8, np.float32, 5, 5, 12, 80, 80, n_cand=9, plant=(1, 2),
                        init=init))
    out.append(Case("maxdiff-skipped-entry", "maxdiff", NCC, np.uint8, np.float32, 5, 5, 7, 80, 80, global_start=1000,
                    cand_offset=5, n_cand=5, cands="edges", plant="skipped"))
    # degenerate patterns, both sides, both metrics: (recipe, degenerate under ncc, degenerate under ndp)
    u8 = [(("random",), False, False), (("const", 0), True, True), (("const", 255), True, False), (("random",), False, False)]
    f32 = [(("random",), False, False), (("const", 0.25), True, False), (("const", 0.0), True, True),
           (("rpoke", np.nan, True), True, True), (("rpoke", np.inf, True), True, True), (("rpoke", -np.inf, True), True, True),
           (("rpoke", np.nan, False), False, False), (("rpoke", np.inf, False), False, False),
           (("rpoke", -np.inf, False), False, False), (("poke", 0.25, np.nan, False), True, False)]
    u16 = [(("random",), False, False), (("poke", 60000, 60001, True), False, False), (("const", 60000), True, False),
           (("poke", 60000, 59999, True), False, False), (("poke", 60000, 60001, False), True, False)]
    # include/kpdi.h's three cases where a verdict on the doubles differs from the float32 screen's (part of the table
    # since the kernel follows the float32 cast): contrast below float32 resolution, squares that overflow, that underflow
    f64v = [(("random",), False, False), (("scaled", 1.0, 1e-10), True, False), (("scaled", 0.0, 1e25), True, True),
            (("scaled", 0.0, 1e-30), True, True)]
    f32v = [f64v[0], f64v[2], f64v[3]]
    for metric in (NCC, NDP):
        for tag, dtype, rows, group in (("u8", np.uint8, u8, "degenerate"), ("f32", np.float32, f32, "degenerate"),
                                        ("u16", np.uint16, u16, "degenerate"), ("verdict-f64", np.float64, f64v, "verdicts"),
                                        ("verdict-f32", np.float32, f32v, "verdicts")):
            recipes = [r[0] for r in rows]
            deg = tuple(r[1 + metric] for r in rows)
            n = len(rows)
            out.append(Case(f"degenerate-{tag}-{names[metric]}", group, metric, (dtype, recipes), (dtype, recipes), n, n, n, 120,
                            90, pix="perm", n_cand=n, cands="all", deg_exp=deg, deg_dic=deg))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = ("dtypes", "lengths", "rows", "window", "maxdiff", "degenerate", "verdicts")
