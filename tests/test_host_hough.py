"""Hough indexing without a GPU: csrc/hough_plan.h and csrc/hough_vote.h under the host compiler
against the NumPy restatement of tests/_hough_restate.py - the Radon sum, the smoothing and the bands bit for bit, the
votes as integers, the fitted orientation to rounding -; hand-made sinograms (a peak on the theta seam with a tie across it,
a plateau, fewer maxima than bands, the rim); synthetic normals with outliers recovered exactly; three wrong variants
that the tables notice; the restatement inside one rho cell of the known orientations of the simulated and of the
reference's experimental Ni patterns; the launch plan; the public signatures and refusals."""

import inspect

import numpy as np
import pytest

import _hough_cases as cases
import _hough_restate as hr
import kikuchipy_amd as kpa
from kikuchipy_amd import _lib
from kikuchipy_amd.indexing import _hough_indexing as hi


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("houghprobe"))
    exe = cases.build_probe(tmp)
    if exe is None:
        pytest.skip("no host C++ compiler")
    return exe, tmp


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def band_table_fails(wrong):
    """Whether the seam case of the hand-made sinograms notices the variant."""
    s = cases.sinogram_cases()["seam_tie"]
    one = np.ones(1, dtype=np.float32)
    g = hr.geometry(60, 60, *s.shape)
    right, _ = hr.bands(s, g, one, one, 1, 3)
    got, _ = hr.bands(s, g, one, one, 1, 3, wrong)
    return not same_bits(right, got)


def normal_table_fails(wrong):
    right = hr.band_normals([0.3, 1.2, 2.9], [5.0, -11.5, 0.25], (0.42, 0.22, 0.5), 60, 60)
    return not np.allclose(right, hr.band_normals([0.3, 1.2, 2.9], [5.0, -11.5, 0.25], (0.42, 0.22, 0.5), 60, 60, wrong), atol=1e-12)


def line_table_fails(wrong):
    """Whether a drawn line comes back more than half a cell from where it was drawn."""
    img = cases.drawn_line((61, 47), 37.0, -6.0)
    plan = cases.indexer((61, 47), (0.5, 0.5, 0.5), nBands=1).bandDetectPlan
    cos_sin, wt, wr, rim = plan.tables()
    g = hr.geometry(61, 47, plan.nTheta, plan.nRho, wrong)
    b, _ = hr.bands(hr.radon(img, g, cos_sin), g, wt, wr, rim, 1, wrong)
    return not (abs(np.degrees(b["theta"][0]) - 37.0) <= 0.5 and abs(b["rho"][0] + 6.0) <= 0.5 * plan.rho_cell)


# ---- the headers against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 5), (60, 60), (61, 47)])
def test_header_radon_and_bands_are_the_restatement(probe, shape):
    exe, tmp = probe
    plan = cases.indexer(shape, (0.5, 0.5, 0.5), nBands=5).bandDetectPlan
    cos_sin, wt, wr, rim = plan.tables()
    g = hr.geometry(*shape, plan.nTheta, plan.nRho)
    for pattern in cases.radon_patterns(shape, np.float32):
        n_mask, s, u, b = cases.probe_bands(exe, tmp, hr.staged(pattern, g), plan.nTheta, plan.nRho, 5, cos_sin, wt, wr, rim)
        want = hr.radon(pattern, g, cos_sin)
        assert n_mask == int(g["mask"].sum())
        assert same_bits(s, want)
        wb, wu = hr.bands(want, g, wt, wr, rim, 5)
        assert same_bits(u, wu)
        assert same_bits(b, wb), (b, wb)


def test_hand_made_sinograms(probe):
    exe, tmp = probe
    one = np.ones(1, dtype=np.float32)
    table = cases.sinogram_cases()
    n_theta, n_rho = table["plateau"].shape
    g = hr.geometry(60, 60, n_theta, n_rho)
    cs = np.zeros((2, n_theta), dtype=np.float32)
    found = {}
    for name, s in table.items():
        b, _ = hr.bands(s, g, one, one, 1, 3)
        _, _, _, pb = cases.probe_bands(exe, tmp, s, n_theta, n_rho, 3, cs, one, one, 1, sinogram=True)
        assert same_bits(b, pb), name
        found[name] = [(int(r["a"]), int(r["k"])) for r in b if r["valid"]]
    assert found["seam_tie"] == [(0, 6)]  # its equal across the seam is in its window and has the higher index
    assert found["plateau"] == [(5, 8)]
    assert found["two_peaks"] == [(3, 5), (12, 14)]
    assert found["rim"] == [(10, 10)]
    smoothed = hr.bands(table["two_peaks"], g, np.array([0.25, 0.5, 0.25], dtype=np.float32), one, 1, 3)[0]
    assert [(int(r["a"]), int(r["k"])) for r in smoothed if r["valid"]] == [(3, 5), (12, 14)]
    assert smoothed["da"][0] == 0 and smoothed["dk"][0] == 0  # symmetric neighbours: the vertex is the cell


def test_a_bright_pixel_gives_its_sinusoid():
    shape, (i0, j0) = (61, 47), (20, 30)
    img = np.zeros(shape, dtype=np.float32)
    img[i0, j0] = 1000.0
    plan = cases.indexer(shape, (0.5, 0.5, 0.5)).bandDetectPlan
    cos_sin = plan.tables()[0]
    g = hr.geometry(*shape, plan.nTheta, plan.nRho)
    s = hr.radon(img, g, cos_sin)
    theta = np.arange(plan.nTheta) * np.pi / plan.nTheta
    rho = np.cos(theta) * (j0 - (shape[1] - 1) / 2) + np.sin(theta) * (i0 - (shape[0] - 1) / 2)
    got = (np.argmax(s, axis=1) - (plan.nRho - 1) / 2) * plan.rho_cell
    assert np.abs(got - rho).max() <= 0.5 * plan.rho_cell + 1e-6


def test_wrong_variants_are_noticed():
    tables = (band_table_fails, normal_table_fails, line_table_fails)
    assert not any(t(None) for t in tables)
    for wrong in cases.WRONG:
        assert any(t(wrong) for t in tables), wrong


def test_header_normal_is_the_restatement(probe):
    exe, tmp = probe
    for theta, rho, pc, shape in ((0.3, 5.0, (0.42, 0.22, 0.5), (60, 60)), (2.9, -17.25, (0.51, 0.48, 0.63), (96, 80))):
        np.testing.assert_allclose(cases.probe_normal(exe, tmp, theta, rho, pc, shape),
                                   hr.band_normals(theta, rho, pc, *shape), rtol=0, atol=1e-14)


def test_synthetic_normals_with_outliers_are_recovered(probe):
    exe, tmp = probe
    normals, q, phase, s2d = cases.synthetic_normals()
    tol = np.deg2rad(2.0)
    votes, quat, fit, nmatch, indexed = cases.probe_index(exe, tmp, normals, phase, tol, s2d)
    ang = hr.np.arccos(np.clip(np.abs(normals @ normals.T), None, 1.0))
    assert np.array_equal(votes, hr.votes(ang, phase.angles, phase.family, int(phase.family.max()) + 1, tol))
    rq, rfit, rn, rok = hr.index(normals, 9, phase.normals, phase.family, phase.angles, tol, s2d)
    assert indexed and rok and nmatch == rn == 6
    assert fit < 1e-5 and rfit < 1e-5
    for got in (quat, rq):
        assert kpa.disorientation_angle(got, q, "432", degrees=True) < 1e-5
    # (exact data: the 24 equivalent hypotheses tie to rounding, so the two may return different equivalents)
    assert kpa.disorientation_angle(quat, rq, "432", degrees=True) < 1e-5
    # too few bands, and bands that are noise: not indexed
    assert not cases.probe_index(exe, tmp, normals[:2], phase, tol, s2d)[4]
    assert hr.index(normals[:2], 9, phase.normals, phase.family, phase.angles, tol, s2d)[3] is False


# ---- known answers on the CPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.SIMULATED_SHAPES)
def test_restatement_is_inside_a_rho_cell_of_the_simulated_truth(shape):
    patterns = cases.simulated_patterns_host(shape)
    q, pcs = cases.simulated_inputs(shape)
    for i in range(cases.N_SIMULATED):
        quat, fit, nmatch, ok, _ = hr.index_pattern(patterns[i], cases.indexer(shape, pcs[i]), pcs[i])
        bound = cases.cell_bound(pcs[i, 2], shape[0])
        off = float(kpa.disorientation_angle(quat, q[i], "432", degrees=True))
        print(shape, i, "disorientation", off, "fit", fit, "nmatch", nmatch, "bound", bound)
        assert ok and off < bound and fit < bound


def test_restatement_is_inside_a_rho_cell_of_the_experimental_truth():
    from oracle import kpdi_oracle as ko

    patterns, bg, pcs, truth = cases.ni_experimental()
    p = ko.remove_dynamic_background(ko.remove_static_background(patterns.reshape(9, 60, 60), bg))
    for i in range(9):
        quat, fit, nmatch, ok, _ = hr.index_pattern(p[i], cases.indexer((60, 60), pcs[i]), pcs[i])
        off = float(kpa.disorientation_angle(quat, truth[i], "432", degrees=True))
        print(i, "disorientation", off, "fit", fit, "nmatch", nmatch)
        assert ok and off < cases.cell_bound(pcs[i, 2], 60)


def test_y_not_negated_misses_the_simulated_truth():
    shape = (60, 60)
    patterns, (q, pcs) = cases.simulated_patterns_host(shape)[:3], cases.simulated_inputs(shape)
    off = [float(kpa.disorientation_angle(hr.index_pattern(patterns[i], cases.indexer(shape, pcs[i]), pcs[i], "y_not_negated")[0],
                                          q[i], "432", degrees=True)) for i in range(3)]
    assert max(off) > cases.cell_bound(0.5, 60)


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def test_plan():
    fits, spills = _lib.hough_plan_describe(201, 201, 180, 201, 2, 1 << 30), _lib.hough_plan_describe(202, 201, 180, 201, 2, 1 << 30)
    assert fits["lds"] == 1 and fits["lds_bytes"] == 201 * 201 * 4 + 2048 <= 160 * 1024
    assert spills["lds"] == 0 and spills["lds_bytes"] == 2048
    assert spills["pattern_bytes"] == 3 * 180 * 201 * 4 + 202 * 201 * 4 and fits["pattern_bytes"] == 3 * 180 * 201 * 4
    assert _lib.hough_plan_describe(240, 240, 180, 239, 1, 1 << 30)["lds"] == 0
    p = _lib.hough_plan_describe(60, 60, 180, 59, 1000, 10 * 3 * 180 * 59 * 4 + 5)
    assert (p["pass_patterns"], p["n_passes"], p["tail_patterns"]) == (10, 100, 10)
    p = _lib.hough_plan_describe(60, 60, 180, 59, 1000, 1 << 40, forced=7)
    assert (p["pass_patterns"], p["n_passes"], p["tail_patterns"]) == (7, 143, 6)
    assert _lib.hough_plan_describe(60, 60, 180, 59, 1000, 100)["ok"] == 0
    assert _lib.hough_plan_describe(2, 60, 180, 59, 1, 1 << 30)["ok"] == 0
    assert _lib.hough_default_n_rho(60, 60) == 59 and _lib.hough_default_n_rho(61, 47) == 47 and _lib.hough_default_n_rho(5, 5) == 5


# ---- the interface ----------------------------------------------------------------------------------------------------------
# parameter names and defaults of the reference's callables (signals/ebsd.py:1600-1728, detectors/_ebsd_detector.py:1598,
# indexing/_hough_indexing.py:43-50, :339-345, :409-413)
SIGNATURES = {
    "EBSD.hough_indexing": (kpa.EBSD.hough_indexing, ["self", "phase_list", "indexer", "chunksize", "verbose", "return_index_data",
                                                      "return_band_data"], [528, 1, False, False]),
    "EBSD.hough_indexing_optimize_pc": (kpa.EBSD.hough_indexing_optimize_pc, ["self", "pc0", "indexer", "batch", "method", "kwargs"],
                                        [False, "Nelder-Mead"]),
    "EBSDDetector.get_indexer": (kpa.EBSDDetector.get_indexer, ["self", "phase_list", "reflectors", "kwargs"], [None]),
    "xmap_from_hough_indexing_data": (hi.xmap_from_hough_indexing_data, ["data", "phase_list", "data_index", "navigation_shape",
                                                                         "step_sizes", "scan_unit"], [-1, None, None, "px"]),
    "_indexer_is_compatible_with_kikuchipy": (hi._indexer_is_compatible_with_kikuchipy,
                                              ["indexer", "sig_shape", "nav_size", "check_pc", "raise_if_not"], [None, True, False]),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signatures(name):
    fn, names, defaults = SIGNATURES[name]
    params = inspect.signature(fn).parameters
    assert list(params) == names
    assert [p.default for p in params.values() if p.default is not inspect.Parameter.empty] == defaults


def test_indexer_attributes_and_refusals():
    det = kpa.EBSDDetector((60, 60), pc=(0.42, 0.22, 0.5), sample_tilt=69.5, tilt=3.0)
    ix = det.get_indexer(cases.POINT_GROUP, nBands=8)
    assert ix.vendor == "KIKUCHIPY" and ix.sampleTilt == 69.5 and ix.camElev == 3.0 and np.array_equal(ix.PC, [0.42, 0.22, 0.5])
    assert ix.bandDetectPlan.patDim == (60, 60) and ix.bandDetectPlan.nBands == 8 and ix.bandDetectPlan.nTheta == 180
    assert len(ix.phaselist) == 1 and ix.phaselist[0].normals.shape == (25, 3) and int(ix.phaselist[0].family.max()) == 3
    with pytest.raises(TypeError, match="backend"):
        det.get_indexer(cases.POINT_GROUP, backend="opencl")
    with pytest.raises(ValueError, match="One set of reflectors or None must be passed per phase"):
        det.get_indexer([cases.POINT_GROUP, cases.POINT_GROUP], reflectors=[[[1, 1, 1]], [[2, 0, 0]], [[2, 2, 0]]])
    # a triclinic lattice goes through the reciprocal basis
    basis = np.array([[0.31, 0.02, -0.01], [-0.05, 0.22, 0.03], [0.04, -0.06, 0.17]])
    tri = det.get_indexer(kpa.Reflectors([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [-1, 0, 0]], None, reciprocal_basis=basis))
    assert tri.phaselist[0].normals.shape == (4, 3) and int(tri.phaselist[0].family.max()) == 3
    s = kpa.EBSD(np.zeros((2, 2, 60, 60), dtype=np.uint8))
    with pytest.raises(ValueError, match="`pc0` must be of size 3"):
        s.hough_indexing_optimize_pc([0.4, 0.2], ix)
    with pytest.raises(ValueError, match="`method` 'powell' must be one of the supported methods"):
        s.hough_indexing_optimize_pc([0.4, 0.2, 0.5], ix, method="Powell")
    with pytest.raises(NotImplementedError, match="PSO"):
        s.hough_indexing_optimize_pc([0.4, 0.2, 0.5], ix, method="PSO")
    with pytest.raises(ValueError, match=r"Indexer signal shape \(60, 60\) must be equal to the signal shape \(50, 60\)"):
        kpa.EBSD(np.zeros((2, 50, 60), dtype=np.uint8)).hough_indexing(cases.POINT_GROUP, ix, verbose=0)
    ix.PC = np.zeros((3, 3))
    with pytest.raises(ValueError, match=r"`indexer.PC` must be an array of shape \(3,\) or \(4, 3\), but was \(3, 3\) instead"):
        s.hough_indexing(cases.POINT_GROUP, ix, verbose=0)
    ix.PC, ix.vendor = np.array([0.42, 0.22, 0.5]), "EDAX"
    with pytest.raises(ValueError, match="'indexer.vendor' must be 'kikuchipy', but was EDAX"):
        s.hough_indexing(cases.POINT_GROUP, ix, verbose=0)
    ix.vendor = "KIKUCHIPY"
    with pytest.raises(ValueError, match=r"`phase_list` \(2\) and `indexer.phaselist` \(1\) have unequal number of phases"):
        s.hough_indexing([cases.POINT_GROUP, cases.POINT_GROUP], ix, verbose=0)


def test_xmap_from_index_data():
    data = np.zeros((2, 6), dtype=hi.INDEX_DTYPE)
    data["quat"][..., 1] = 1.0
    data["phase"][:, :4] = 0
    data["phase"][:, 4:] = -1
    data["fit"] = np.arange(6)
    xmap = hi.xmap_from_hough_indexing_data(data, cases.POINT_GROUP, navigation_shape=(2, 3))
    assert xmap.shape == (2, 3) and xmap.size == 6 and xmap.is_in_data.all()
    assert np.array_equal(xmap.phase_id, [0, 0, 0, 0, -1, -1])
    assert np.array_equal(xmap.rotations[4:], [[1, 0, 0, 0]] * 2) and np.array_equal(xmap.rotations[0], [0, 1, 0, 0])
    assert np.array_equal(xmap.get_map_data("fit"), np.arange(6.0).reshape(2, 3))
    with pytest.raises(ValueError, match="`nav_shape` cannot be a tuple of more than two integers"):
        hi.xmap_from_hough_indexing_data(data, cases.POINT_GROUP, navigation_shape=(1, 2, 3))
    with pytest.raises(ValueError, match=r"`phase_list` IDs \[0\] must contain 1"):
        hi.xmap_from_hough_indexing_data(data, cases.POINT_GROUP, data_index=1)
