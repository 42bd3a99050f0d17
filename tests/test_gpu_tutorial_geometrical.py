"""Where tests/test_gpu_tutorial_walkthrough.py stops, the reference's pattern-matching tutorial
(doc/tutorials/pattern_matching.ipynb) goes on: the geometrical simulation of the refined orientations on the refined
detector, to be laid over the patterns.  The nine Ni patterns are indexed and refined as there, then
`KikuchiPatternSimulator.on_detector` projects the Ni reflectors of the kinematical fixtures for the (3, 3) map."""

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def test_geometrical_simulation_of_the_refined_map():
    import kikuchipy_amd as kp
    from kikuchipy_amd import sampling

    pre, proj = load_golden("preproc.npz"), load_golden("projection.npz")
    s = kp.signals.EBSD(pre["ni"].copy(), static_background=pre["ni_bg"])
    s.remove_static_background()
    s.remove_dynamic_background()
    energy = 20
    mp = kp.signals.EBSDMasterPattern(np.stack([proj["mp_upper"], proj["mp_lower"]])[:, None], energies=[energy],
                                      hemisphere="both", projection="lambert")
    R = sampling.get_sample_fundamental(method="cubochoric", resolution=6, point_group="m-3m")
    det = kp.detectors.EBSDDetector(shape=s.axes_manager.signal_shape[::-1], pc=[0.4198, 0.2136, 0.5015], sample_tilt=70)
    sim = mp.get_patterns(rotations=R, detector=det, energy=energy, dtype_out=np.float32, compute=True)
    signal_mask = ~kp.filters.Window("circular", det.shape).astype(bool)
    xmap = s.dictionary_indexing(sim, metric="ncc", keep_n=20, signal_mask=signal_mask, verbose=False)
    xmap_ref = s.refine_orientation(xmap=xmap, detector=det, master_pattern=mp, energy=energy, signal_mask=signal_mask,
                                    verbose=False)
    result_arr = s.refine_projection_center(xmap=xmap, detector=det, master_pattern=mp, energy=energy,
                                            signal_mask=signal_mask, method="minimize",
                                            method_kwargs=dict(method="Powell", tol=1e-3), trust_region=[0.02, 0.02, 0.02],
                                            compute=False, verbose=False)
    _, det_ref, _ = kp.indexing.compute_refine_projection_center_results(results=result_arr, detector=det, xmap=xmap)
    assert det_ref.navigation_shape == (3, 3)
    rot = np.asarray(xmap_ref.rotations).reshape(3, 3, 4)
    # the geometrical simulation
    ni = load_golden("kinematical.npz")
    reflectors = kp.Reflectors(ni["in__ni__hkl"], ni["in__ni__theta"], ni["in__ni__structure_factor"], phase_name="ni")
    simulation = kp.KikuchiPatternSimulator(reflectors).on_detector(det_ref, rot)
    assert simulation.navigation_shape == (3, 3) and simulation.ndim == 2
    assert 0 < simulation.reflectors.size <= reflectors.size and simulation.zone_axes.shape[0] > 0
    lines = simulation.lines_coordinates((1, 1))
    zone_axes = simulation.zone_axes_coordinates((1, 1))
    assert lines.ndim == 2 and lines.shape[1] == 4 and lines.shape[0] > 0 and not np.isnan(lines).any()
    assert zone_axes.ndim == 2 and zone_axes.shape[1] == 2 and zone_axes.shape[0] > 0 and not np.isnan(zone_axes).any()
    # zone axes lie inside the detector widened by one pixel
    x0, x1, y0, y1 = det_ref.bounds
    tiny = 1e-9
    assert (zone_axes[:, 0] >= x0 - 1 - tiny).all() and (zone_axes[:, 0] <= x1 + 1 + tiny).all()
    assert (zone_axes[:, 1] >= y0 - 1 - tiny).all() and (zone_axes[:, 1] <= y1 + 1 + tiny).all()
    # without NaN exclusion every index gives the same shape
    shapes = {(simulation.lines_coordinates(i, exclude_nan=False).shape, simulation.zone_axes_coordinates(i, exclude_nan=False).shape)
              for i in np.ndindex(3, 3)}
    assert shapes == {((simulation.reflectors.size, 4), (simulation.zone_axes.shape[0], 2))}
    assert simulation.lines_coordinates((1, 1), "gnomonic").shape == lines.shape
