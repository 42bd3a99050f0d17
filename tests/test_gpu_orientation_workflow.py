"""The cells that follow indexing and refinement in the reference's material, on this package:

(a) the known answer of the reference's refinement benchmark (benchmarks/indexing/test_refinement.py:25-85): the nine Ni
    patterns with static and dynamic background removed, the Ni master pattern, `EBSDDetector(shape=(60, 60),
    pc=(0.42, 0.22, 0.50), sample_tilt=70)`, the circular mask, the benchmark's two start orientations,
    `refine_orientation` with its defaults, then `xmap_ref.rotations.angle_with(rot, degrees=True) < 0.8` at every point;
(b) the pattern-matching tutorial's `Or.angle_with(O_ref, degrees=True)` between the indexed and the refined map
    (doc/tutorials/pattern_matching.ipynb), on the walkthrough's small dictionary: with m-3m the angles are at most the
    plain rotation angles, and equal the minimum over the 24 explicit equivalents."""

import numpy as np
import pytest

import _orientation_cases as cases
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nickel():
    import kikuchipy_amd as kp

    pre, proj = load_golden("preproc.npz"), load_golden("projection.npz")
    s = kp.signals.EBSD(pre["ni"].copy(), static_background=pre["ni_bg"])
    s.remove_static_background()
    s.remove_dynamic_background()
    mp = kp.signals.EBSDMasterPattern(np.stack([proj["mp_upper"], proj["mp_lower"]])[:, None], energies=[20],
                                      hemisphere="both", projection="lambert")
    return s, mp


def test_refinement_benchmark_known_answer(nickel):
    import kikuchipy_amd as kp
    from kikuchipy_amd.indexing._refinement import rotation_from_euler

    s, mp = nickel
    rot1, rot2 = np.deg2rad([258, 58, 1]), np.deg2rad([292, 62, 182])
    rot = rotation_from_euler(np.array([rot1, rot2, rot2, rot1, rot2, rot2, rot1, rot2, rot2]))
    detector = kp.detectors.EBSDDetector(shape=(60, 60), pc=(0.42, 0.22, 0.50), sample_tilt=70)
    signal_mask = ~kp.filters.Window("circular", (60, 60)).astype(bool)
    xmap_ref = s.refine_orientation(xmap=rot, detector=detector, master_pattern=mp, energy=20, signal_mask=signal_mask)
    angles = kp.disorientation_angle(xmap_ref.rotations, rot, "1", degrees=True, device=0)
    print("angles between the refined and the start orientations (degrees):", angles)
    assert angles.shape == (9,) and np.all(angles < 0.8)
    assert np.array_equal(angles, kp.disorientation_angle(xmap_ref, rot, degrees=True, device=0))  # a result holder, the default group


def test_tutorial_angles_between_indexed_and_refined_maps(nickel):
    import kikuchipy_amd as kp
    from kikuchipy_amd import sampling

    s, mp = nickel
    R = sampling.get_sample_fundamental(method="cubochoric", resolution=6, point_group="m-3m")
    det = kp.detectors.EBSDDetector(shape=(60, 60), pc=[0.4198, 0.2136, 0.5015], sample_tilt=70)
    sim = mp.get_patterns(rotations=R, detector=det, energy=20, dtype_out=np.float32, compute=True)
    signal_mask = ~kp.filters.Window("circular", det.shape).astype(bool)
    xmap = s.dictionary_indexing(sim, metric="ncc", keep_n=20, signal_mask=signal_mask, verbose=False)
    xmap_ref = s.refine_orientation(xmap=xmap, detector=det, master_pattern=mp, energy=20, signal_mask=signal_mask, verbose=False)
    best = np.asarray(xmap.rotations)[:, 0]
    assert best.shape == (9, 4) and np.asarray(xmap_ref.rotations).shape == (9, 4)
    with kp._lib.Context(0) as ctx:
        cubic = kp.disorientation_angle(best, xmap_ref.rotations, "m-3m", degrees=True, context=ctx)
        plain = kp.disorientation_angle(best, xmap_ref.rotations, "1", degrees=True, context=ctx)
        ops = sampling.rotation_group_operations("432")
        explicit = np.stack([kp.disorientation_angle(sampling.quaternion_product(op, best), xmap_ref.rotations, "1", degrees=True,
                                                     context=ctx) for op in ops])
        # every top-k candidate against the refined orientation: (9, 20, 4) against (9, 1, 4)
        topk = kp.disorientation_angle(xmap.rotations, np.asarray(xmap_ref.rotations)[:, None, :], "m-3m", degrees=True, context=ctx)
    print("m-3m:", cubic, "\n1:   ", plain)
    bound = 2 * cases.angle_bound(0.0, degrees=True)  # two computed angles are compared
    assert (cubic <= plain + bound).all()
    assert explicit.shape == (24, 9) and (np.abs(cubic - explicit.min(axis=0)) <= bound).all()
    assert topk.shape == (9, 20) and np.array_equal(topk[:, 0], cubic)
