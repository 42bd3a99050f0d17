"""`EBSDDetector.estimate_xtilt`, `estimate_xtilt_ztilt`, `fit_pc`, `extrapolate_pc` and the PC conventions (DESIGN.md
section 28) against tests/golden/pc_fit.npz, which tools/gen_pc_fit_golden.py wrote by running the reference's
detectors/_fit_projection_center.py and detector methods.  No GPU.

Tolerances.  The fits solve least-squares problems whose index matrices have condition numbers below ~1e3, so two LAPACK
builds differ by around 1e-13: 1e-10 absolute on PCs and on tilts in radians leaves three orders of magnitude and is
still 1e-8 of a pixel.  `extrapolate_pc` and the conversions are elementwise: 1e-14 absolute on values of order 1 (the
EMsoft convention holds pixels and microns, up to ~3e4: 1e-14 relative there)."""

import inspect
import json
import os
import warnings

import numpy as np
import pytest

import kikuchipy_amd as kpa
from kikuchipy_amd import _pc_fit

FIT_ATOL = 1e-10
ELEMENTWISE_ATOL = 1e-14
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pc_fit.npz"))
# the projective fit of the 1-D grid is not among them: a line of map points determines no homography, the reference's
# result there is not a fit (tools/gen_pc_fit_golden.py) and this package refuses (test_refusals_and_warnings)
FIT_CASES = [f"{g}_{t}_{m}_{o}" for g, ts in (("g5", ("projective", "affine")), ("g7", ("affine",))) for t in ts
             for m in ("map2", "map3") for o in ("all", "masked")]


def detector(pc, **kwargs):
    d = json.loads(str(GOLDEN["detector"]))
    d.update(kwargs)
    return kpa.EBSDDetector(tuple(d.pop("shape")), pc=pc, **d)


def test_golden_holds_every_case():
    assert sorted(json.loads(str(GOLDEN["fit_cases"]))) == sorted(FIT_CASES)
    assert "robust_is_outlier" in GOLDEN.files and "scikit-learn 0.24.2" in str(GOLDEN["made_by"])
    assert GOLDEN["g5_pc"].shape == (5, 5, 3) and GOLDEN["g7_pc"].shape == (7, 3)
    assert GOLDEN["g5_map2"].ndim == 2 and GOLDEN["g5_map3"].ndim == 3


@pytest.mark.parametrize("case", FIT_CASES)
def test_fit_pc(case):
    grid, transformation, map_form, masked = case.split("_")
    det = detector(GOLDEN[grid + "_pc"])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        new = det.fit_pc(GOLDEN[grid + "_pc_indices"], GOLDEN[f"{grid}_{map_form}"], transformation=transformation,
                         is_outlier=GOLDEN[grid + "_is_outlier"] if masked == "masked" else None)
    want = GOLDEN[case + "_pc"]
    assert new.pc.shape == want.shape == GOLDEN[f"{grid}_{map_form}"].shape[1:] + (3,)
    x_tilt = np.deg2rad(90 - new.sample_tilt - new.tilt)
    dev_pc, dev_tilt = float(np.abs(new.pc - want).max()), abs(x_tilt - float(GOLDEN[case + "_xtilt"]))
    print(case, "largest PC deviation", dev_pc, "tilt deviation [rad]", dev_tilt)
    assert dev_pc <= FIT_ATOL and dev_tilt <= FIT_ATOL
    assert new.shape == det.shape and new.tilt == det.tilt and new.navigation_shape == want.shape[:-1]
    assert det.sample_tilt == 70.0  # the detector itself is left alone


@pytest.mark.parametrize("grid", ["g5", "g7"])
def test_estimate_tilts(grid):
    det = detector(GOLDEN[grid + "_pc"])
    got = det.estimate_xtilt()  # plot=True by default: accepted, nothing drawn
    dev = [abs(got - float(GOLDEN[grid + "_xtilt_linear"]))]
    assert isinstance(got, float) and det.estimate_xtilt(degrees=True) == float(np.rad2deg(got))
    assert det.estimate_xtilt(plot=False, figure_kwargs={"figsize": (3, 3)}) == got
    for masked in ("all", "masked"):
        xz = det.estimate_xtilt_ztilt(is_outlier=GOLDEN[grid + "_is_outlier"] if masked == "masked" else None)
        dev.append(float(np.abs(np.array(xz) - GOLDEN[f"{grid}_xz_{masked}"]).max()))
    print(grid, "tilt deviations [rad]", dev)
    assert max(dev) <= FIT_ATOL
    xz_deg = det.estimate_xtilt_ztilt(degrees=True)
    assert np.allclose(np.deg2rad(xz_deg), det.estimate_xtilt_ztilt(), rtol=0, atol=1e-15)
    # the plane was made as `extrapolate_pc` makes one, at alpha = 90 - 70 + 3 degrees: the slope of PCy on PCz gives it back
    if grid == "g5":
        assert abs(np.rad2deg(got) - (90 - 70 + 3)) < 1.0


def test_robust_fit_names_the_reference_outliers():
    det = detector(GOLDEN["robust_pc"])
    want = GOLDEN["robust_is_outlier"]
    assert want.sum() == 3 and want.shape == (5, 5)
    x_tilt, is_outlier = det.estimate_xtilt(detect_outliers=True, return_outliers=True)
    assert is_outlier.dtype == bool and np.array_equal(is_outlier, want)
    dev = abs(x_tilt - float(GOLDEN["robust_xtilt"]))
    print("robust tilt deviation [rad]", dev)
    assert dev <= FIT_ATOL
    assert det.estimate_xtilt(return_outliers=True)[0] == x_tilt  # return_outliers implies detect_outliers
    assert len(det.estimate_xtilt(detect_outliers=True)) == 2  # as in the reference: the mask comes with the robust fit
    assert abs(det.estimate_xtilt() - x_tilt) > 1e-3  # the plain fit is pulled by the outliers
    # deterministic, and ties go to the first pair: the same call twice, and a permutation-free statement of the rule
    assert np.array_equal(det.estimate_xtilt(return_outliers=True)[1], want)
    x, y = np.array([0.0, 1.0, 2.0, 3.0, 4.0]), np.array([0.0, 1.0, 2.0, 3.0, 40.0])
    slope, intercept, inlier = _pc_fit.robust_linear_fit(x, y)
    assert list(inlier) == [True, True, True, True, False] and slope == 1.0 and intercept == 0.0
    with pytest.raises(ValueError, match="no consensus set"):
        _pc_fit.robust_linear_fit(x, np.zeros(5))


def test_extrapolate_pc():
    det = detector(GOLDEN["g5_pc"])
    indices = GOLDEN["extrapolate_indices"]
    assert indices[0].min() < 0 and indices[1].max() > 40  # outside the 31 x 41 map
    for case, kwargs in (("plain", {}), ("given", dict(shape=(120, 100), px_size=35.0, binning=2)),
                         ("masked", dict(is_outlier=GOLDEN["g5_is_outlier"].ravel()))):
        new = det.extrapolate_pc(indices, (31, 41), (1.5, 2.0), **kwargs)
        want = GOLDEN[f"extrapolate_{case}_pc"]
        dev = float(np.abs(new.pc - want).max())
        print("extrapolate", case, "largest deviation", dev)
        assert new.pc.shape == want.shape == (31, 41, 3) and dev <= ELEMENTWISE_ATOL
        meta = json.loads(str(GOLDEN[f"extrapolate_{case}_detector"]))
        assert (list(new.shape), new.px_size, new.binning) == (list(meta["shape"]), meta["px_size"], meta["binning"])
        assert new.sample_tilt == det.sample_tilt and new.tilt == det.tilt
    assert det.shape == (60, 60) and det.navigation_shape == (5, 5)


def test_conventions_and_round_trip():
    meta = json.loads(str(GOLDEN["convention_detector"]))
    pc = GOLDEN["g5_pc"]
    det = kpa.EBSDDetector(tuple(meta["shape"]), px_size=meta["px_size"], binning=meta["binning"], pc=pc)
    tall = kpa.EBSDDetector((80, 60), pc=pc)
    got = {"emsoft4": det.pc_emsoft(4), "emsoft5": det.pc_emsoft(), "tsl": det.pc_tsl(), "oxford": det.pc_oxford(),
           "tall_tsl": tall.pc_tsl(), "tall_oxford": tall.pc_oxford()}
    for name, value in got.items():
        want = GOLDEN["convention_" + name]
        dev = float(np.abs(value - want).max() / max(1.0, np.abs(want).max()))
        print(name, "largest deviation", dev)
        assert value.shape == want.shape == (5, 5, 3) and dev <= ELEMENTWISE_ATOL
    assert det.pc_bruker() is det.pc and np.array_equal(det.pc, pc)  # nothing above wrote into the detector
    assert np.array_equal(got["emsoft4"][..., 0], -got["emsoft5"][..., 0])
    # back through the constructor
    for d, conventions in ((det, ("emsoft4", "emsoft5", "tsl", "oxford")), (tall, ("tsl", "oxford"))):
        for convention in conventions:
            value = got[("tall_" if d is tall else "") + convention]
            back = kpa.EBSDDetector(d.shape, px_size=d.px_size, binning=d.binning, pc=value, convention=convention)
            assert np.abs(back.pc - pc).max() <= 1e-15 * 4, convention
    one = kpa.EBSDDetector((60, 80), pc=(0.4, 0.2, 0.6), px_size=59.2, binning=8)  # the reference's docstring examples
    assert np.allclose(one.pc_emsoft(), [[64.0, 144.0, 17049.6]], rtol=1e-15, atol=0)
    assert np.allclose(one.pc_emsoft(4), [[-64.0, 144.0, 17049.6]], rtol=1e-15, atol=0)
    assert np.allclose(one.pc_tsl(), [[0.4, 0.8, 0.6]], rtol=1e-15, atol=0)


def test_refusals_and_warnings():
    det = detector(GOLDEN["g5_pc"])
    idx, mask = GOLDEN["g5_pc_indices"], GOLDEN["g5_is_outlier"]
    one = detector((0.5, 0.2, 0.5))
    with pytest.raises(ValueError, match="Estimation requires more than one projection center"):
        one.estimate_xtilt()
    with pytest.raises(ValueError, match="Estimation requires more than one projection center"):
        one.estimate_xtilt_ztilt()
    with pytest.raises(ValueError, match=r"Fitting requires multiple projection centers \(PCs\)"):
        one.fit_pc([[0], [0]], idx.reshape(2, -1))
    with pytest.raises(ValueError, match=r"`pc_indices` array shape \(2, 25\) must be equal to \(2, 5, 5\)"):
        det.fit_pc(idx.reshape(2, -1), idx)
    with pytest.raises(ValueError, match=r"`map_indices` array shape \(3, 5, 5\) must be \(2, m columns\) or \(2, n rows, m columns\)"):
        det.fit_pc(idx, np.zeros((3, 5, 5)))
    with pytest.raises(ValueError, match=r"`map_indices` array shape \(2,\) must be"):
        det.fit_pc(idx, np.zeros(2))
    line = detector(GOLDEN["g7_pc"])
    with pytest.raises(ValueError, match="lie on a line, which determines no homography; use transformation='affine'"):
        line.fit_pc(GOLDEN["g7_pc_indices"], GOLDEN["g7_map2"])
    for bad in (mask.astype(int), mask[:4], list(mask.ravel())):
        with pytest.raises(ValueError, match="`is_outlier` must be a boolean array of a size equal to the number of PCs"):
            det.fit_pc(idx, idx, is_outlier=bad)
    for call in (lambda: det.fit_pc(idx, idx, return_figure=True), lambda: det.estimate_xtilt(return_figure=True)):
        with pytest.raises(NotImplementedError, match="needs Matplotlib, which this package does not use"):
            call()
    turned = detector(GOLDEN["g5_pc"], azimuthal=1.5, twist=-0.5)
    tail = r" azimuthal=1.5 and twist=-0.5 will be ignored\."
    for text, call in (
            (r"estimate_xtilt\(\) assumes azimuthal and twist angles are zero, but", turned.estimate_xtilt),
            (r"estimate_xtilt_ztilt\(\) assumes azimuthal and twist angles are zero, but", turned.estimate_xtilt_ztilt),
            (r"extrapolate_pc\(\) assumes azimuthal and twist angles are zero, but",
             lambda: turned.extrapolate_pc(idx.reshape(2, -1), (3, 3), (1, 1))),
            (r"fit_pc\(\) assumes azimuthal and twist angles are zero when estimating sample_tilt, but",
             lambda: turned.fit_pc(idx, idx))):
        with pytest.warns(UserWarning, match=text + tail):
            call()


def test_signatures_are_the_reference_s():
    table = json.loads(str(GOLDEN["signatures"]))
    assert sorted(table) == ["estimate_xtilt", "estimate_xtilt_ztilt", "extrapolate_pc", "fit_pc", "pc_bruker", "pc_emsoft",
                             "pc_oxford", "pc_tsl"]
    assert [n for n, _ in table["estimate_xtilt"]] == ["detect_outliers", "plot", "degrees", "return_figure", "return_outliers",
                                                       "figure_kwargs"]
    for name, want in table.items():
        params = list(inspect.signature(getattr(kpa.EBSDDetector, name)).parameters.values())[1:]
        got = [[p.name, "<required>" if p.default is inspect.Parameter.empty else p.default] for p in params]
        assert got == want, name
        assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params), name
