"""rescore_kernel on its own (csrc/rescore.hip through kpdi_rescore_selftest): every case of tests/_rescore_cases.py - all
81 pairs of raw dtypes under both metrics, the reduction lengths around the kernel's strides of 64 and 256 with and
without a pix_map, row maps, every edge of the candidate window, max_diff from every wave and workgroup, degenerate
patterns on both sides - against the np.longdouble evaluation of the reference's formula: scores to 1e-12 (the float64
path's contract, TOL of tests/test_gpu_f64.py), degenerate entries exactly +0.0, skipped entries exactly -inf, everything
outside the window bit for bit what the caller put there, max_diff to 2 float32 ulps.
tests/test_host_rescore_cases.py shows that a kernel wrong in any of nineteen named ways would fail here.

Then the degeneracy verdict end to end (include/kpdi.h "Degenerate patterns": taken on the float32 cast, independent of
chunking): patterns that are ordinary in double and degenerate in float32 score 0 whether their chunk is small enough to
be rescored completely or not."""
import numpy as np
import pytest

import _rescore_cases as R
from kikuchipy_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def run(ctx, b, **over):
    c = b.case
    kw = dict(cand_offset=c.cand_offset, n_cand=c.n_cand, global_start=c.global_start, row_map=b.row_map, pix_map=b.pix_map,
              k=b.k, max_diff=b.init)
    kw.update(over)
    return ctx.rescore_selftest(b.exp, b.dic, c.metric, b.cand_s, b.cand_i, kw.pop("out", b.fill.copy()), **kw)


@pytest.mark.parametrize("group", R.GROUPS)
def test_every_case_against_the_precise_reference(ctx, group):
    complaints, worst, at = [], 0.0, None
    for c in R.CASES:
        if c.group != group:
            continue
        b = R.build(c.name)
        got, md, err = run(ctx, b)
        assert err == 0, (c.name, err)
        bad, w = R.check(b, got, md)
        complaints += [(c.name, line) for line in bad]
        if w >= worst:
            worst, at = w, c.name
    print(f"{group}: worst |score - reference| {worst:.3e} ({at})")  # shown with the failure, and by pytest -rP
    assert not complaints, (f"worst {worst:.3e}", len(complaints), complaints[:6])


def test_what_would_read_outside_a_buffer_is_refused_before_the_launch(ctx):
    b = R.build("rows-3-of-17")
    c = b.case

    def refused(match, **over):
        out = b.fill.copy()
        with pytest.raises(_lib.KpdiError, match=match):
            run(ctx, b, out=out, **over)
        assert (out.view(np.uint64) == np.uint64(R.FILL_BITS)).all()

    refused("row_map", row_map=[16, 17, 9])
    refused("row_map", row_map=[16, -1, 9])
    pix = b.pix_map.copy()
    pix[-1] = c.npix
    refused("pix_map", pix_map=pix)
    pix[-1] = -1
    refused("pix_map", pix_map=pix)
    refused("cand_stride", n_cand=c.n_cand + c.pad + 1)
    refused("cand_stride", cand_offset=c.pad + 1)
    refused("cand_stride", cand_offset=-1)
    refused("k must be", k=0)
    refused("k must be", k=-3)
    for code in (-1, 9, 100):
        refused("dtype", exp_dtype=code)
        refused("dtype", dict_dtype=code)
    refused("pix_map", pix_map=None, k=c.npix + 1)  # without a map the first k pixels: no more than there are
    got, md, err = run(ctx, b)  # and the context is as good as before
    assert err == 0 and not R.check(b, got, md)[0]


# ---- the two verdicts ---------------------------------------------------------------------------------------------------
def probe_pattern(kind, u, dtype):
    """A pattern whose float32 verdict is "degenerate" and whose float64 arithmetic is perfectly ordinary, from u in
    [0, 1): contrast below float32 resolution / centred squares that overflow float32 / that underflow it - each orders
    of magnitude from where summation order could decide."""
    return {"contrast": 1.0 + 1e-10 * u, "overflow": 1e25 * u, "underflow": 1e-30 * u}[kind].astype(dtype)


PROBES = [("contrast", np.float64, "ncc"), ("overflow", np.float32, "ncc"), ("overflow", np.float64, "ncc"),
          ("underflow", np.float32, "ncc"), ("underflow", np.float64, "ncc"), ("overflow", np.float32, "ndp"),
          ("underflow", np.float64, "ndp")]


@pytest.mark.parametrize("kind,dtype,metric", PROBES)
def test_the_float32_verdict_holds_whatever_the_chunk_size(kind, dtype, metric):
    """A 30-pattern dictionary is rescored completely (30 <= keep_n + 12); inside 600 patterns the float32 screen alone
    decides who is rescored.  Dictionary pattern 7 is experimental pattern 0 itself, made degenerate-in-float32: in double
    it would correlate perfectly.  Experimental pattern 1 is such a pattern too."""
    import kikuchipy_amd as ka

    rng = np.random.default_rng(17)
    m, s, keep_n, at = 6, 20, 20, 7
    u = rng.random((m, s, s))
    exp = u.astype(dtype)
    exp[1] = probe_pattern(kind, u[1], dtype)
    small = (0.6 * u[np.arange(30) % m] + 0.4 * rng.random((30, s, s))).astype(dtype)  # five real matches per pattern
    small[at] = probe_pattern(kind, u[0], dtype)
    large = np.concatenate([small, rng.random((570, s, s)).astype(dtype)])
    res = {}
    for name, dic in (("small", small), ("large", large)):
        r = ka.dictionary_indexing(exp, dic, metric, keep_n, n_per_iteration=len(dic), dtype=np.float64, device=0, verbose=False)
        assert r.float64_certificate["uncertified_patterns"] == 0, (name, r.float64_certificate)
        sc, ix = r.scores, r.simulation_indices
        assert sc.dtype == np.float64 and np.isfinite(sc).all()
        assert (sc[ix == at] == 0).all() and not np.signbit(sc[ix == at]).any(), (name, sc[ix == at])
        assert (ix[:, 0] != at).all(), (name, ix[:, 0])
        assert np.array_equal(sc[1], np.zeros(keep_n)) and np.array_equal(ix[1], np.arange(keep_n)), (name, sc[1], ix[1])
        res[name] = (sc, ix)
    (ss, si), (ls, li) = res["small"], res["large"]
    if metric == "ncc":  # fewer than 20 of 29 real scores are positive: the small run must show it, with its 0
        assert (np.delete(si, 1, axis=0) == at).any()
    shared = 0
    for r in range(m):
        for a_s, a_i, b_s, b_i in ((ss[r], si[r], ls[r], li[r]), (ls[r], li[r], ss[r], si[r])):
            for sc, ix in zip(a_s, a_i):
                if sc > 0 and ix < 30 and ix in b_i:
                    assert abs(b_s[list(b_i).index(ix)] - sc) <= R.TOL, (r, ix, sc)
                    shared += 1
    assert shared >= 2 * 5 * (m - 1)  # the real matches are in both results
