"""The Radon and the band kernel of Hough indexing (csrc/hough.hip) on the GPU against the NumPy restatement of
tests/_hough_restate.py, bit for bit: 5 x 5, 60 x 60, 61 x 47 and 202 x 201 patterns - the last the smallest shape beside
201 x 201 whose staged pattern does not fit in LDS -, 131 x 129 (more LDS than a kernel gets without asking), uint8, uint16
and float32, forced passes; a bright pixel's sinusoid; drawn lines - one in the open, one on the theta seam, two that tie,
one alone for nine bands -; constant and NaN patterns; the refusals of the C ABI."""

import numpy as np
import pytest

import _hough_cases as cases
import _hough_restate as hr
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with _lib.Context(0) as c:
        yield c


def detect(ctx, patterns, plan, sinograms=True):
    sy, sx = patterns.shape[-2:]
    ctx.set_problem(sy, sx, None, _lib.METRIC_NCC, 1)
    ctx.set_experimental(patterns.reshape(-1, sy, sx))
    cos_sin, wt, wr, rim = plan.tables()
    return ctx.hough_bands(plan.nRho, cos_sin, wt, wr, rim, plan.nBands, sinograms)


def restated(patterns, plan):
    cos_sin, wt, wr, rim = plan.tables()
    g = hr.geometry(*patterns.shape[-2:], plan.nTheta, plan.nRho)
    sino = np.stack([hr.radon(p, g, cos_sin) for p in patterns])
    return np.stack([hr.bands(s, g, wt, wr, rim, plan.nBands)[0] for s in sino]), sino


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


SHAPES = [(5, 5), (60, 60), (61, 47), (202, 201)]


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32"])
@pytest.mark.parametrize("shape", SHAPES)
def test_radon_and_bands_bit_for_bit(ctx, shape, dtype):
    plan = cases.indexer(shape, (0.5, 0.5, 0.5), nBands=5).bandDetectPlan
    assert _lib.hough_plan_describe(*shape, plan.nTheta, plan.nRho, 2, 1 << 30)["lds"] == (shape != (202, 201))
    patterns = cases.radon_patterns(shape, dtype)
    bands, sino = detect(ctx, patterns, plan)
    want_bands, want_sino = restated(patterns, plan)
    assert same_bits(sino, want_sino)
    assert same_bits(bands, want_bands)


def test_radon_with_more_lds_than_the_default(ctx):
    shape = (131, 129)
    plan = cases.indexer(shape, (0.5, 0.5, 0.5), nBands=5).bandDetectPlan
    p = _lib.hough_plan_describe(*shape, plan.nTheta, plan.nRho, 1, 1 << 30)
    assert p["lds"] == 1 and p["lds_bytes"] > 64 * 1024
    patterns = cases.radon_patterns(shape, np.float32, n=1)
    bands, sino = detect(ctx, patterns, plan)
    want_bands, want_sino = restated(patterns, plan)
    assert same_bits(sino, want_sino) and same_bits(bands, want_bands)


def test_passes_do_not_change_the_bits(ctx, monkeypatch):
    plan = cases.indexer((61, 47), (0.5, 0.5, 0.5), nBands=5).bandDetectPlan
    patterns = cases.radon_patterns((61, 47), np.uint8, n=5)
    bands, sino = detect(ctx, patterns, plan)
    monkeypatch.setenv("KPDI_HOUGH_PASS", "2")
    bands2, sino2 = detect(ctx, patterns, plan)
    assert same_bits(sino, sino2) and same_bits(bands, bands2)


def test_a_bright_pixel_gives_its_sinusoid(ctx):
    shape, (i0, j0) = (61, 47), (20, 30)
    img = np.zeros((1,) + shape, dtype=np.float32)
    img[0, i0, j0] = 1000.0
    plan = cases.indexer(shape, (0.5, 0.5, 0.5)).bandDetectPlan
    _, sino = detect(ctx, img, plan)
    theta = np.arange(plan.nTheta) * np.pi / plan.nTheta
    rho = np.cos(theta) * (j0 - (shape[1] - 1) / 2) + np.sin(theta) * (i0 - (shape[0] - 1) / 2)
    got = (np.argmax(sino[0], axis=1) - (plan.nRho - 1) / 2) * plan.rho_cell
    assert np.abs(got - rho).max() <= 0.5 * plan.rho_cell + 1e-6


def test_drawn_lines(ctx):
    shape = (61, 47)
    plan = cases.indexer(shape, (0.5, 0.5, 0.5)).bandDetectPlan  # nine bands asked for
    lines = [(37.0, -6.0), (0.0, 4.0), (179.6, -9.0), (90.0, 11.0)]
    tie = np.maximum(cases.drawn_line(shape, 90.0, 11.0), cases.drawn_line(shape, 90.0, -11.0))  # mirror images: a tie
    patterns = np.stack([cases.drawn_line(shape, t, r) for t, r in lines] + [tie])
    bands = detect(ctx, patterns, plan, sinograms=False)
    want, _ = restated(patterns, plan)
    assert same_bits(bands, want)
    for b, (t, r) in zip(bands, lines):
        assert b["valid"][0] == 1
        dt = abs(np.degrees(b["theta"][0]) - t)
        if min(dt, 180 - dt) > 0.5:
            raise AssertionError((b[0], t, r))
        flipped = dt > 90  # found across the seam: the same line with rho negated
        assert abs(b["rho"][0] - (-r if flipped else r)) <= 0.5 * plan.rho_cell
    assert (bands["valid"].sum(axis=1) >= 1).all()
    assert sorted(abs(float(v)) for v in bands[4]["rho"][:2]) == pytest.approx([11.0, 11.0], abs=0.5 * plan.rho_cell)


def test_constant_and_nan_patterns_are_not_indexed(ctx):
    shape = (60, 60)
    patterns = cases.radon_patterns(shape, np.float32, n=3)
    patterns[0] = 7.0
    patterns[1, 10, 10] = np.nan
    s = kpa.EBSD(patterns)
    try:
        ix = cases.indexer(shape, (0.42, 0.22, 0.5))
        xmap, index_data, band_data = s.hough_indexing(cases.POINT_GROUP, ix, verbose=0, return_index_data=True, return_band_data=True)
    finally:
        s.close()
    assert band_data.shape == (3, 9) and index_data.shape == (2, 3)
    assert (band_data["valid"][:2] == 0).all() and band_data["valid"][2].any()
    assert list(xmap.phase_id[:2]) == [-1, -1] and np.array_equal(xmap.rotations[:2], [[1, 0, 0, 0]] * 2)
    assert (index_data["nmatch"][:, :2] == 0).all() and (index_data["fit"][:, :2] == 180).all()


def test_c_abi_refusals(ctx):
    plan = cases.indexer((60, 60), (0.5, 0.5, 0.5)).bandDetectPlan
    cos_sin, wt, wr, rim = plan.tables()
    ctx.set_problem(60, 60, None, _lib.METRIC_NCC, 1)
    ctx.set_experimental(cases.radon_patterns((60, 60), np.uint8))
    for kwargs in (dict(n_bands=0), dict(n_bands=17), dict(rim=0), dict(rim=30), dict(n_rho=2)):
        args = dict(n_rho=plan.nRho, cos_sin=cos_sin, theta_taps=wt, rho_taps=wr, rim=rim, n_bands=9)
        args.update(kwargs)
        with pytest.raises(_lib.KpdiError):
            ctx.hough_bands(**args)
    with pytest.raises(_lib.KpdiError):
        ctx.hough_bands(plan.nRho, cos_sin, np.ones(35, dtype=np.float32), wr, rim, 9)
    bands = ctx.hough_bands(plan.nRho, cos_sin, wt, wr, rim, 9)
    phase = cases.indexer((60, 60), (0.5, 0.5, 0.5)).phaselist[0]
    s2d = np.eye(3)
    with pytest.raises(_lib.KpdiError):
        ctx.hough_index(bands, np.zeros((3, 3)) + 0.5, (60, 60), s2d, phase.normals, phase.family, phase.angles, 0.05)
    with pytest.raises(_lib.KpdiError):
        ctx.hough_index(bands, [0.5, 0.5, 0.5], (60, 60), s2d, phase.normals, phase.family, phase.angles, 0.0)
