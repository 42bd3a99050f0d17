"""Pixel probes for every preparation kernel path (csrc/prep.hip, chosen by csrc/prep_plan.h): the case table, the probe
builder and a float64 reference.  Pure NumPy, seeded, no GPU.  tests/test_host_prep_cases.py checks on the CPU that the table
reaches every kernel family (with prep_plan.h compiled by the host compiler), that the builder is right and that every case
is sensitive to one misplaced pixel; tests/test_gpu_prep_matrix.py runs the table through the engine.

A ONE-HOT pattern scored against pattern x returns (a known multiple of) the prepared, normalised value of that one pixel of
x, so a pixel that a kernel drops, duplicates or moves shows up in the probe standing on it at 200 - 2000 times the 1e-5
tolerance, where a random-against-random score moves by 1 / K.  A probe on a masked-out pixel is all zero under the mask:
degenerate, exactly +0 against everything.

Every case is swept twice: side "a" - the probes are the experimental set, the patterns the dictionary (keep_n = number of
patterns); side "b" - the patterns are the experimental set (with a navigation mask in every third case), the probes the
dictionary (keep_n = number of probes).  The full score matrix is put together again from (scores, indices) and compared
entry by entry, so tie order never matters.

len(CASES) = 502 cases (x 2 sides), counted by test_host_prep_cases.py::test_case_count.

Shapes.  Candidates of the issue plus 120 x 120 and 150 x 150: with an unmasked 128 x 128 detector the wide float32 form pads
K = 16 384 to 16 392 columns and falls to the generic kernel, so 120 x 120 is its largest workgroup-per-pattern shape, and a
circular mask on 150 x 150 keeps 17 660 pixels - the cheapest masked shape beyond the workgroup kernels.  (The float16 form
counts `kpad` in PAIRS of pixels, so its span 2 * kpad is K rounded up to 48 and its size classes change at the same K as
the other forms', not at half of it.)

Tolerance.  Forms 0, 1 and 3: the project's contract, 1e-5 against float64.  Form 2 (float16 operands, reduced precision):
per case, twice the largest deviation from the exact float64 scores of a float64 evaluation whose prepared operands are
rounded to float16(2^12 * value) (tests/test_gpu_f16.py) - the factor 2 for a value whose float32
preparation lands on the other side of a float16 rounding boundary, and for the accumulation order.  Largest value per
shape over the cases of the table (test_host_prep_cases.py::test_float16_tolerances prints them):
FORM2_TOLERANCES below.  The sensitivity condition (a probe moved to the adjacent kept pixel changes >= 90 % of its scores
by more than 10 x the tolerance) holds at every shape with these values, so no shape is dropped for form 2.
"""
import collections
import functools
import zlib

import numpy as np

ATOL = 1e-5  # README "Parity"
SEED = "prep-probes-2:"  # of every case's patterns (changed until every case met the sensitivity condition)
DTYPES = ("uint8", "int8", "uint16", "int16", "int32", "uint32", "float16", "float32", "float64")
FORMS = {"f32": 0, "f16x2": 1, "f16": 2, "wide": 3}  # compute name -> operand form (`counters()["match_form"]`)
METRICS = ("ncc", "ndp")
KEPT_PROBES = (0, 1, 3, 4, 31, 32, 63, 64, 255, 256, 4095, 4096)  # quad, slab, wave and size-class boundaries
# largest form-2 tolerance of the table per detector shape (see the module docstring); test_host_prep_cases.py::
# test_float16_tolerances keeps them within 10 % above what the cases give (24 x 20: the five-pixel mask, whose values are large)
FORM2_TOLERANCES = {
    (8, 8): 2.4e-4, (24, 20): 7.1e-4, (45, 45): 8.2e-5, (60, 60): 5.6e-5, (64, 64): 4.1e-5, (64, 65): 2.8e-5, (75, 75): 4.5e-5,
    (90, 91): 3.4e-5, (120, 120): 1.75e-5, (128, 128): 1.85e-5, (128, 129): 1.15e-5, (130, 130): 1.3e-5, (150, 150): 1.7e-5,
    (256, 250): 9.3e-6,
}

Case = collections.namedtuple("Case", "shape mask metric compute dtype variant n push env nav")
# mask: none / crop / circ / scatter / keep5 / keep1;  variant: "" or "top" (32-bit integers that use the top byte)
# push: host / dev0 / dev1 (device pointer offset by 0 / 1 elements) / devb4 / devb8 / devb12 (float32: by bytes) / held
# env: tuple of (name, value) switches;  nav: side "b" carries a navigation mask


def case_id(c):
    env = "".join(f"-{k[5:]}={v}" for k, v in c.env)
    return (f"{c.shape[0]}x{c.shape[1]}-{c.mask}-{c.metric}-{c.compute}-{c.dtype}{c.variant and '-' + c.variant}-n{c.n}-{c.push}"
            f"{env}{'-nav' if c.nav else ''}")


def _table():
    out, seen = [], set()

    def add(shape, mask, metric, compute, dtype, variant="", n=None, push="host", env=()):
        i = len(out)
        c = Case(tuple(shape), mask, metric, compute, dtype, variant, n or (37, 69)[i % 2], push, tuple(env), i % 3 == 0)
        if case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)

    # 1. every size class and its boundaries, every form, both metrics; the dtype rotates.  Small masked detectors
    # also as float32: the gather and LDS-DMA kernels take float32 rows only.
    scen = [((8, 8), "none"), ((24, 20), "none"), ((24, 20), "crop"), ((45, 45), "none"), ((45, 45), "circ"),
            ((60, 60), "none"), ((60, 60), "crop"), ((60, 60), "circ"), ((60, 60), "scatter"), ((64, 64), "none"),
            ((64, 64), "circ"), ((64, 65), "none"), ((64, 65), "crop"), ((75, 75), "none"), ((75, 75), "scatter"),
            ((90, 91), "none"), ((90, 91), "circ"), ((120, 120), "none"), ((128, 128), "none"), ((128, 128), "circ"),
            ((128, 129), "none"), ((130, 130), "none"), ((150, 150), "circ")]
    j = 0
    for compute in FORMS:
        for metric in METRICS:
            for shape, mask in scen:
                d = DTYPES[j % 9]
                j += 1
                add(shape, mask, metric, compute, d if d != "float32" or mask == "none" else "int16")
                if mask != "none" and shape[0] * shape[1] <= 4096:
                    add(shape, mask, metric, compute, "float32")
    # 2. every dtype (and the top-byte variants) through every family of forms 0 and 3
    fam = [((60, 60), "none"), ((45, 45), "none"), ((60, 60), "scatter"), ((64, 65), "none"), ((90, 91), "circ"),
           ((75, 75), "none")]
    for compute in ("f32", "wide"):
        for fi, (shape, mask) in enumerate(fam):
            for di, (d, v) in enumerate([(d, "") for d in DTYPES] + [("int32", "top"), ("uint32", "top")]):
                add(shape, mask, METRICS[(fi + di) % 2], compute, d, v)
    # 3. raw pointers that are not 16-byte aligned (device pushes, never coalesced)
    for compute in ("f32", "wide", "f16", "f16x2"):
        for push in ("dev0", "devb4", "devb8", "devb12"):
            add((60, 60), "crop", "ncc", compute, "float32", push=push)
            add((60, 60), "scatter", "ndp", compute, "float32", push=push)
    for di, d in enumerate(DTYPES):
        for push in ("dev0", "dev1"):
            add((60, 60), "none", METRICS[di % 2], "f32", d, push=push)
            add((64, 65), "none", METRICS[(di + 1) % 2], "wide", d, push=push)
    for push in ("dev0", "dev1"):
        add((60, 60), "circ", "ncc", "f16", "uint8", push=push)
        add((64, 65), "none", "ndp", "f16", "uint16", push=push)
        add((64, 65), "none", "ncc", "f16x2", "int8", push=push)
    # 4. the fallbacks behind the switches, where they change the plan
    for metric in METRICS:
        for compute in ("f32", "wide"):
            add((60, 60), "scatter", metric, compute, "uint8", env=[("KPDI_PREP_NO_STAGED", "1")])
            add((60, 60), "scatter", metric, compute, "float32", env=[("KPDI_PREP_NO_DMA", "1")])
            add((60, 60), "crop", metric, compute, "float32", env=[("KPDI_PREP_NO_GATHER", "1")])
            add((60, 60), "crop", metric, compute, "float32", env=[("KPDI_PREP_NO_GATHER", "1"), ("KPDI_PREP_NO_DMA", "1")])
        for compute in ("wide", "f16"):
            add((60, 60), "none", metric, compute, "uint8", env=[("KPDI_PREP_NO_LINES", "1")])
            add((60, 60), "crop", metric, compute, "float32", env=[("KPDI_PREP_NO_LINES", "1")])
        for v in ("block", "block4"):
            add((64, 65), "none", metric, "f16", "uint8", env=[("KPDI_PREP16", v)])
            add((90, 91), "circ", metric, "f16", "float32", env=[("KPDI_PREP16", v)])
    # 5. held chunks, the smallest masks, one pattern, the largest detector
    for ci, compute in enumerate(FORMS):
        add((60, 60), "circ", METRICS[ci % 2], compute, "float32", push="held")
        add((90, 91), "none", METRICS[(ci + 1) % 2], compute, "uint8", push="held")
        for metric in METRICS:
            add((24, 20), "keep5", metric, compute, "uint16")
            add((24, 20), "keep1", metric, compute, "float32")
        add((60, 60), "circ", "ncc", compute, "uint16", n=1)
        add((256, 250), "none", METRICS[ci % 2], compute, "uint8", n=69)  # (69: at K = 64 000 a count of uint8 is 3e-5)
        add((256, 250), "circ", METRICS[(ci + 1) % 2], compute, "float32", n=69)
    return out


CASES = _table()


# ---- masks (True = excluded, as the reference's signal_mask) -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def signal_mask(shape, kind):
    sy, sx = shape
    if kind == "none":
        return None
    m = np.zeros(shape, dtype=bool)
    if kind == "crop":  # run-structured: whole rows and a column band (tests/test_gpu_tail.py)
        m[:4] = True
        m[:, :3] = True
    elif kind == "circ":
        yy, xx = np.mgrid[:sy, :sx]
        m = (yy - sy / 2) ** 2 + (xx - sx / 2) ** 2 > (min(sy, sx) / 2) ** 2
    elif kind == "scatter":  # ~30 % excluded at random: a general pixel map
        m = np.random.default_rng(sy * 1000 + sx).random(shape) < 0.3
    elif kind in ("keep5", "keep1"):
        m[:] = True
        m.ravel()[[7, 8, sx + 3, 5 * sx + 1, sy * sx - 2][: 5 if kind == "keep5" else 1]] = False
    else:
        raise ValueError(kind)
    m.setflags(write=False)
    return m


def kept_pixels(shape, kind):
    m = signal_mask(shape, kind)
    return np.arange(shape[0] * shape[1]) if m is None else np.flatnonzero(~m.ravel())


# ---- patterns under test ---------------------------------------------------------------------------------------------
def patterns(c):
    """(n, sy, sx) of the case's dtype: random, exactly representable in float32, negatives where the type has them."""
    # (seeded by what the values depend on: the same patterns however they are pushed and whatever the switches)
    rng = np.random.default_rng(zlib.crc32((SEED + case_id(c._replace(push="host", env=(), nav=False))).encode()))
    size = (c.n,) + c.shape
    d = np.dtype(c.dtype)
    if c.variant == "top":  # multiples of 2^8 up to 2^31: 24 significant bits, the top byte in use
        lo = -(1 << 23) if d.kind == "i" else 0
        return (rng.integers(lo, 1 << 23 if d.kind == "i" else 1 << 24, size) * 256).astype(d)
    if d.kind in "iu":
        bits = min(8 * d.itemsize, 20)  # 32-bit integers: 20 bits, exact in float32 with room for their sums
        lo, hi = (-(1 << (bits - 1)), 1 << (bits - 1)) if d.kind == "i" else (0, 1 << bits)
        return rng.integers(lo, hi, size).astype(d)
    x = rng.standard_normal(size).astype(np.float16 if d == np.float16 else np.float32)
    return x.astype(d)


# ---- probes ----------------------------------------------------------------------------------------------------------
Probe = collections.namedtuple("Probe", "name pixels values kind kept_index")  # kind: kept / out / double


def probe_list(shape, kind):
    """The probes of a detector shape and mask, duplicates (small K) dropped."""
    sy, sx = shape
    mask = signal_mask(shape, kind)
    keep = kept_pixels(shape, kind)
    K = len(keep)
    out, seen = [], set()

    def add(name, pixels, values, pk, ki=None):
        key = (tuple(pixels), tuple(values))
        if key not in seen:
            seen.add(key)
            out.append(Probe(name, tuple(int(p) for p in pixels), tuple(values), pk, ki))

    for j in KEPT_PROBES:
        if j < K:
            add(f"kept{j}", [keep[j]], [1.0], "kept", j)
    for j in range(max(K - 5, 0), K):
        add(f"last{K - 1 - j}", [keep[j]], [1.0], "kept", j)
    if mask is not None:
        flat = mask.ravel()
        cut = [r for r in range(sy) if 0 < mask[r].sum() < sx]
        if cut:  # a detector row that the mask cuts: its first and last kept pixel
            r = cut[len(cut) // 2]
            cols = np.flatnonzero(~mask[r])
            for name, col in (("rowfirst", cols[0]), ("rowlast", cols[-1])):
                p = r * sx + col
                add(name, [p], [1.0], "kept", int(np.searchsorted(keep, p)))
        gone = np.flatnonzero(flat)
        add("out_first", [gone[0]], [1.0], "out")
        add("out_last", [gone[-1]], [1.0], "out")
        beside = [p for p in gone if (p + 1 < sy * sx and not flat[p + 1]) or (p > 0 and not flat[p - 1])]
        add("out_beside", [beside[len(beside) // 2]], [1.0], "out")
    if K >= 2:  # two hot pixels far apart, of unequal height
        add("double0", [keep[K // 7], keep[K - 1 - K // 5]], [1.0, 2.0], "double")
        add("double1", [keep[min(1, K - 1)], keep[K // 2]], [2.0, 1.0], "double")
    return out


def probe_patterns(shape, plist, displaced=False, kind=None):
    """(p, sy, sx) float32.  `displaced`: every single kept-pixel probe stands on the ADJACENT kept pixel instead."""
    out = np.zeros((len(plist), shape[0] * shape[1]), dtype=np.float32)
    keep = kept_pixels(shape, kind) if displaced else None
    for i, p in enumerate(plist):
        pixels = p.pixels
        if displaced and p.kind == "kept" and len(keep) > 1:
            j = p.kept_index
            pixels = (int(keep[j + 1 if j + 1 < len(keep) else j - 1]),)
        out[i, list(pixels)] = p.values
    return out.reshape((len(plist),) + tuple(shape))


Built = collections.namedtuple("Built", "mask keep patterns probes plist nav")


@functools.lru_cache(maxsize=4)
def build(c):
    plist = probe_list(c.shape, c.mask)
    nav = None
    if c.nav and c.n > 3:
        nav = np.zeros(c.n, dtype=bool)
        nav[[2, c.n - 1]] = True
    return Built(signal_mask(c.shape, c.mask), kept_pixels(c.shape, c.mask), patterns(c),
                 probe_patterns(c.shape, plist), plist, nav)


def sides(c, b, side):
    """(experimental set, dictionary, navigation mask) of a side."""
    return (b.probes, b.patterns, None) if side == "a" else (b.patterns, b.probes, b.nav)


# ---- float64 reference -----------------------------------------------------------------------------------------------
def prepared(raw, keep, metric):
    """Rows of `raw` as the reference prepares them, in float64: cast to float32 first, kept pixels, ncc: centre, divide by
    the norm; a row that is constant (ncc), all zero, or not finite becomes the zero row."""
    x = np.asarray(raw).reshape(len(raw), -1).astype(np.float32).astype(np.float64)[:, keep]
    lo, hi = x.min(axis=1), x.max(axis=1)
    if metric == "ncc":
        x = x - x.mean(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = np.sum(x * x, axis=1)
        bad = ~(np.isfinite(n2) & (n2 > 0)) | ((lo == hi) if metric == "ncc" else False)
        out = x / np.sqrt(np.where(bad, 1.0, n2))[:, None]
    out[bad] = 0.0
    return out


def reference(c, b, side, probes=None, float16=False):
    """Full float64 score matrix (experimental rows the navigation mask keeps) x (dictionary).  `float16`: the prepared
    operands rounded as KPDI_COMPUTE_F16 rounds them."""
    exp, dic, nav = sides(c, b, side)
    if probes is not None:
        exp, dic = (probes, dic) if side == "a" else (exp, probes)
    if nav is not None:
        exp = exp[~nav]
    e, d = prepared(exp, b.keep, c.metric), prepared(dic, b.keep, c.metric)
    if float16:
        e, d = ((v * 4096).astype(np.float32).astype(np.float16).astype(np.float64) for v in (e, d))
        return (e @ d.T) * 2.0 ** -24
    return e @ d.T


def tolerance(c, b, side):
    if FORMS[c.compute] != 2:
        return ATOL
    return 2.0 * float(np.abs(reference(c, b, side, float16=True) - reference(c, b, side)).max())


def zero_entries(c, b, side):
    """Boolean matrix: entries that are exactly +0 (a degenerate row on either side)."""
    exp, dic, nav = sides(c, b, side)
    if nav is not None:
        exp = exp[~nav]
    e, d = prepared(exp, b.keep, c.metric), prepared(dic, b.keep, c.metric)
    return ~e.any(axis=1)[:, None] | ~d.any(axis=1)[None, :]


def assemble(scores, indices, n):
    """(m, n) matrix from the (scores, indices) of a sweep that kept all n dictionary entries."""
    assert scores.shape == indices.shape == (len(scores), n)
    assert np.array_equal(np.sort(indices, axis=1), np.broadcast_to(np.arange(n), indices.shape)), "an index is missing"
    full = np.empty(scores.shape, dtype=scores.dtype)
    np.put_along_axis(full, indices, scores, axis=1)
    return full


# ---- pairs of runs that differ only in how the bytes are loaded -------------------------------------------------------
# Listed after reading the kernels: both members give every lane the same kept pixels (quad 4 * (lane + 64 i)), add them in
# the same order and share normalise_and_store_quads, so their prepared rows - and the scores - are the same bits.
#   * a device pointer and a host push of the same values (the same plan);
#   * prep_wave_gather_kernel from a base at +4 / +8 / +12 bytes and from an aligned one;
#   * prep_wave_gather_kernel, prep_wave_masked_dma_kernel and prep_wave_masked_kernel (s += (a + b) + (c + d) per quad);
#   * prep_wave_lines_kernel and prep_wave_kernel<T, 4, true> (sequential sum of the quad's elements in both);
#   * prep16_block4_kernel with NP = 2 and NP = 4 (the same code per 256-thread group).
# NOT in the list (another order of the sums: tolerance only): element-wise against vector loads (prep_wave_kernel<T, 1> /
# prep_kernel after an odd offset), KPDI_PREP_NO_STAGED, KPDI_PREP16=block (prep_block_kernel against prep16_block4_kernel).
def _pair(base, **change):
    return base, base._replace(**change)


def identity_pairs():
    out = []
    g = Case((60, 60), "crop", "ncc", "f32", "float32", "", 37, "dev0", (), False)
    for compute in FORMS:
        gc = g._replace(compute=compute)
        out += [_pair(gc, push="host"), _pair(gc, push="devb4"), _pair(gc, push="devb8"), _pair(gc, push="devb12"),
                _pair(gc, env=(("KPDI_PREP_NO_GATHER", "1"),)),
                _pair(gc, env=(("KPDI_PREP_NO_GATHER", "1"), ("KPDI_PREP_NO_DMA", "1")))]
        out.append(_pair(gc._replace(metric="ndp", mask="circ", n=69), env=(("KPDI_PREP_NO_GATHER", "1"),)))
    s = Case((60, 60), "scatter", "ndp", "f32", "float32", "", 69, "host", (), False)
    out += [_pair(s, env=(("KPDI_PREP_NO_DMA", "1"),)), _pair(s._replace(compute="wide"), env=(("KPDI_PREP_NO_DMA", "1"),))]
    for compute in ("wide", "f16"):
        for metric in METRICS:
            out.append(_pair(Case((60, 60), "none", metric, compute, "uint8", "", 37, "host", (), False),
                             env=(("KPDI_PREP_NO_LINES", "1"),)))
    for shape, mask, d in (((64, 65), "none", "uint8"), ((90, 91), "circ", "float32")):
        out.append(_pair(Case(shape, mask, "ncc", "f16", d, "", 37, "host", (), False), env=(("KPDI_PREP16", "block4"),)))
    return out


IDENTITY_PAIRS = identity_pairs()
