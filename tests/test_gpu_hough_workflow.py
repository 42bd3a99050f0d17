"""Hough indexing end to end on the GPU: simulated Ni patterns of known orientation on three
detectors, host-backed and resident, inside one rho cell; the indexing kernel against the restatement's vote and fit; the
reference's nine experimental Ni patterns inside one rho cell of the orientations stored with them; and the projection
centre search on simulated patterns with a known PC and on the Ni patterns with the reference's tolerances."""

import numpy as np
import pytest

import _hough_cases as cases
import _hough_restate as hr
import kikuchipy_amd as kpa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def master():
    mpu, mpl = cases.master_pattern()
    return kpa.EBSDMasterPattern(np.stack([mpu, mpl]), hemisphere="both")


def simulated(master, shape, pcs=None):
    q, own = cases.simulated_inputs(shape)
    pcs = own if pcs is None else pcs
    det = kpa.EBSDDetector(shape, pc=pcs)
    return master.get_patterns(q, det, compute=True), det, q


@pytest.mark.parametrize("shape", cases.SIMULATED_SHAPES)
def test_simulated_known_answer(master, shape):
    s, det, q = simulated(master, shape)
    ix = det.get_indexer(cases.POINT_GROUP)
    try:
        xmap, index_data, band_data = s.hough_indexing(cases.POINT_GROUP, ix, verbose=0, return_index_data=True, return_band_data=True)
        assert not s.is_resident
        s.to_device()
        resident = s.hough_indexing(cases.POINT_GROUP, ix, verbose=0)
        assert s.is_resident
    finally:
        s.close()
    assert np.array_equal(resident.rotations, xmap.rotations) and np.array_equal(resident.fit, xmap.fit)
    assert xmap.shape == (cases.N_SIMULATED,) and band_data.shape == (cases.N_SIMULATED, 9) and index_data.shape == (2, cases.N_SIMULATED)
    off = kpa.disorientation_angle(xmap.rotations, q, "432", degrees=True)
    bound = np.array([cases.cell_bound(pc[2], shape[0]) for pc in det.pc_flattened])
    print(shape, "disorientation", off, "fit", xmap.fit, "nmatch", xmap.nmatch, "bound", bound)
    assert (xmap.phase_id == 0).all()
    assert (off < bound).all() and (xmap.fit < bound).all()
    # the indexing kernel against the restatement, on the bands the GPU found
    phase = ix.phaselist[0]
    for i in range(0, cases.N_SIMULATED, 4):
        b = band_data[i][band_data[i]["valid"] != 0]
        n = hr.band_normals(b["theta"], b["rho"], det.pc_flattened[i], *shape)
        quat, fit, nmatch, ok = hr.index(n, 9, phase.normals, phase.family, phase.angles, ix.tolerance(ix.PC), ix.sample_to_detector)
        assert ok and nmatch == xmap.nmatch[i] and abs(fit - xmap.fit[i]) < 1e-4
        # (the 24 equivalent hypotheses score the same but for rounding: the two may settle on different equivalents)
        assert kpa.disorientation_angle(quat, xmap.rotations[i], "432", degrees=True) < 1e-4


def ni_signal():
    patterns, bg, pcs, truth = cases.ni_experimental()
    s = kpa.EBSD(patterns, static_background=bg)
    s.remove_static_background()
    s.remove_dynamic_background()
    return s, pcs, truth


def test_experimental_known_answer():
    s, pcs, truth = ni_signal()
    det = kpa.EBSDDetector((60, 60), pc=pcs.reshape(3, 3, 3))
    try:
        xmap = s.hough_indexing(cases.POINT_GROUP, det.get_indexer(cases.POINT_GROUP), verbose=0)
    finally:
        s.close()
    off = kpa.disorientation_angle(xmap.rotations, truth, "432", degrees=True)
    print("disorientation", off, "fit", xmap.fit, "nmatch", xmap.nmatch, "below one degree:", int((off < 1).sum()), "of 9")
    assert xmap.shape == (3, 3) and (xmap.phase_id == 0).all()
    assert (off < np.array([cases.cell_bound(pc[2], 60) for pc in pcs])).all()


def test_optimize_pc_simulated(master):
    shape, pc_true = (120, 120), np.array([0.43, 0.21, 0.51])
    s, det, q = simulated(master, shape, pc_true)
    ix = det.get_indexer(cases.POINT_GROUP)
    pc0 = pc_true + np.array([3.0, -3.0, 3.0]) / shape[0]
    try:
        new = s.hough_indexing_optimize_pc(pc0, ix)
        fits = []
        for pc in (pc0, new.pc_average):
            ix.PC = np.asarray(pc)
            fits.append(float(np.mean(s.hough_indexing(cases.POINT_GROUP, ix, verbose=0).fit)))
    finally:
        s.close()
    print("start", pc0, "found", new.pc_average, "off [px]", (new.pc_average - pc_true) * shape[0], "mean fit", fits)
    assert new.navigation_shape == (1,) and new.shape == shape
    assert np.abs(new.pc_average - pc_true).max() < 1.0 / shape[0]
    assert fits[1] < fits[0]


def test_optimize_pc_experimental():
    s, pcs, _ = ni_signal()
    det0 = kpa.EBSDDetector((60, 60), pc=pcs.reshape(3, 3, 3))
    ix = det0.get_indexer(cases.POINT_GROUP)
    try:
        det = s.hough_indexing_optimize_pc(det0.pc_average, ix)
        det2 = s.hough_indexing_optimize_pc(det0.pc_average, ix, batch=True)
    finally:
        s.close()
    print("average", det0.pc_average, "found", det.pc_average, "batch", det2.pc_average)
    assert det.navigation_shape == (1,) and det2.navigation_shape == (3, 3)
    assert np.allclose(det.pc_average, det0.pc_average, atol=0.05)
    assert np.allclose(det.pc_average, det2.pc_average, atol=0.1)
    assert det.shape == det0.shape and det.sample_tilt == det0.sample_tilt and det.tilt == det0.tilt
