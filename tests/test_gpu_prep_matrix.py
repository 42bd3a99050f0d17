"""Every preparation kernel path of csrc/prep.hip against a float64 reference, pixel by pixel: the case table of
tests/_prep_cases.py (one-hot probe patterns; tests/test_host_prep_cases.py shows on the CPU which kernel each case runs and
that one misplaced pixel moves a probe's scores by more than 10 x the tolerance), one small sweep per case and side.

Forms 0, 1 and 3: |score - float64 reference| <= 1e-5, the project's contract.  Form 2 (float16 operands): twice the
deviation of the float16-rounded float64 evaluation, per case (_prep_cases.tolerance).  Entries with a degenerate pattern on
either side - a probe on a masked-out pixel, a one-pixel mask under ncc - are exactly +0.  Runs that differ only in how the
bytes are loaded (_prep_cases.IDENTITY_PAIRS) return the same bits."""
import numpy as np
import pytest

import _prep_cases as P

pytestmark = pytest.mark.gpu

SWITCHES = ("KPDI_F32_WIDE", "KPDI_TAIL_GEMM", "KPDI_NO_COALESCE", "KPDI_PREP_NO_STAGED", "KPDI_PREP_NO_LINES",
            "KPDI_PREP_NO_DMA", "KPDI_PREP_NO_GATHER", "KPDI_PREP16")


def push_device(ctx, array, offset_bytes, call):
    """`array` from a device allocation, `offset_bytes` behind a 256-byte boundary; `call(pointer)` hands it over."""
    a = np.ascontiguousarray(array)
    base = ctx.dev_alloc(a.nbytes + 256)
    try:
        assert base % 256 == 0
        ctx.h2d(base + offset_bytes, a)
        call(base + offset_bytes)
        ctx.synchronize()
    finally:
        ctx.dev_free(base)


def sweep(monkeypatch, c, side):
    """(full score matrix, scores, indices) of one side of a case; a fresh context per switch setting: KPDI_F32_WIDE and
    KPDI_NO_COALESCE are read at set_problem, the KPDI_PREP_* switches at every preparation launch."""
    from kikuchipy_amd import _lib

    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if c.compute in ("f32", "wide"):
        monkeypatch.setenv("KPDI_F32_WIDE", "1" if c.compute == "wide" else "0")
    device = c.push.startswith("dev")
    if device:
        monkeypatch.setenv("KPDI_NO_COALESCE", "1")  # a small chunk would be copied into the coalescing buffer first
    for k, v in c.env:
        monkeypatch.setenv(k, v)
    b = P.build(c)
    exp, dic, nav = P.sides(c, b, side)
    keep_n = len(dic)
    compute = {"f32": _lib.COMPUTE_F32, "wide": _lib.COMPUTE_F32, "f16x2": _lib.COMPUTE_F16X2, "f16": _lib.COMPUTE_F16}[c.compute]
    es = np.dtype(c.dtype).itemsize
    offset = {"dev1": es, "devb4": 4, "devb8": 8, "devb12": 12}.get(c.push, 0)
    with _lib.Context(0) as ctx:
        ctx.set_problem(c.shape[0], c.shape[1], b.mask, {"ncc": _lib.METRIC_NCC, "ndp": _lib.METRIC_NDP}[c.metric], keep_n,
                        compute)
        if device and side == "b":
            push_device(ctx, exp, offset, lambda p: ctx.set_experimental_dev(p, exp.dtype, len(exp), nav))
        else:
            ctx.set_experimental(exp, nav)
        if device and side == "a":
            push_device(ctx, dic, offset, lambda p: ctx.push_dictionary_chunk_dev(p, dic.dtype, len(dic), 0))
        elif c.push == "held":
            ctx.hold_dictionary_chunk(dic, 0)
            ctx.sweep_held()
        else:
            ctx.push_dictionary_chunk(dic, 0)
        s, i = ctx.finalize(keep_n)
        assert ctx.counters()["match_form"] == P.FORMS[c.compute]
    return P.assemble(s, i, keep_n), s, i


@pytest.mark.parametrize("side", "ab")
@pytest.mark.parametrize("c", P.CASES, ids=P.case_id)
def test_probe_scores(monkeypatch, c, side):
    b = P.build(c)
    got, _, _ = sweep(monkeypatch, c, side)
    want = P.reference(c, b, side)
    assert got.shape == want.shape
    tol = P.tolerance(c, b, side)
    err = np.abs(got.astype(np.float64) - want)
    if not (err <= tol).all():
        r, q = np.unravel_index(np.argmax(err), err.shape)
        probe = b.plist[r if side == "a" else q]
        pytest.fail(f"{P.case_id(c)}/{side}: |score - float64| = {err.max():.3g} > {tol:.3g} at probe {probe.name} "
                    f"(pixels {probe.pixels}), pattern {q if side == 'a' else r}; probes off: "
                    f"{sorted({b.plist[j].name for j in np.unique(np.nonzero(err > tol)[0 if side == 'a' else 1])})}")
    zero = P.zero_entries(c, b, side)
    assert (got[zero] == 0).all() and not np.signbit(got[zero]).any()
    if c.mask == "keep1":  # one kept pixel: ncc has nothing left, ndp is the sign of the pixel (+-1 within the tolerance above)
        assert zero.all() if c.metric == "ncc" else (np.abs(want[~zero]) == 1).all() and (np.sign(got) == np.sign(want)).all()


@pytest.mark.parametrize("side", "ab")
@pytest.mark.parametrize("pair", P.IDENTITY_PAIRS, ids=lambda p: P.case_id(p[0]) + "=" + P.case_id(p[1]).split("-n")[1])
def test_same_bits_however_the_bytes_are_loaded(monkeypatch, pair, side):
    x, y = pair
    _, sx, ix = sweep(monkeypatch, x, side)
    _, sy, iy = sweep(monkeypatch, y, side)
    assert np.array_equal(sx.view(np.uint32), sy.view(np.uint32)) and np.array_equal(ix, iy)
